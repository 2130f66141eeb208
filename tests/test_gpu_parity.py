"""GPU parity tests proper: the HIP path, called through the C ABI, against the
CPU oracle on the same seeded inputs.  Bit-exact for neighbour indices, labels,
plane lists, centres; normals bit-exact as well (shared deterministic acos/cos,
contraction off) -- the north-star tolerance of 1e-5 is asserted first and the
exact comparison second so a failure says which bar was missed."""
import numpy as np
import pytest

from buildingsegment_amd import api, synth

pytestmark = pytest.mark.gpu


def _check_knn_normals(ctx, O, xyz, k, **kw):
    p = api.default_params(k=k, **kw)
    neigh, normals = ctx.knn_normals(xyz, p)
    oneigh, onormals = O.knn_normals(xyz, k=k, radius=p.radius, max_nn=p.max_nn)
    assert np.array_equal(neigh, oneigh), f"{(neigh != oneigh).any(axis=1).sum()} rows differ"
    assert np.abs(normals - onormals).max() <= 1e-5  # north-star tolerance
    assert np.array_equal(normals, onormals)
    return neigh, normals


RG_MODES = (1, 2)  # 1 = single-wave sequential, 2 = multi-plane speculative (the default)


def _check_grow(ctx, O, xyz, normals, neigh, **kw):
    out = None
    for mode in RG_MODES:
        out = _check_grow_mode(ctx, O, xyz, normals, neigh, mode, **kw)
    return out


def _check_grow_mode(ctx, O, xyz, normals, neigh, mode, **kw):
    p = api.default_params(k=neigh.shape[1], rg_mode=mode, **kw)
    plane_idx, planes = ctx.region_grow(xyz, normals, neigh, p)
    opi, opl = O.region_grow(xyz, normals, neigh, th_thickness=p.th_thickness,
                             th_point_count=p.th_point_count, cos_th=p.cos_th)
    assert np.array_equal(plane_idx, opi), f"{(plane_idx != opi).sum()} labels differ"
    assert len(planes) == len(opl["id"])
    for i, pl in enumerate(planes):
        assert pl.id == opl["id"][i]
        assert np.array_equal(pl.pointIdx, opl["point_idx"][opl["offset"][i]:opl["offset"][i + 1]])
        assert np.array_equal(pl.center, opl["center"][i])
        assert np.array_equal(pl.normal, opl["normal"][i])
    return plane_idx, planes


def test_plane_cube_100k_reference_literals(gpu_ctx, oracle):
    xyz = synth.plane_cube()
    neigh, normals = _check_knn_normals(gpu_ctx, oracle, xyz, 15)
    plane_idx, planes = _check_grow(gpu_ctx, oracle, xyz, normals, neigh)
    assert len(planes) >= 1 and (plane_idx > 0).sum() > 60000


@pytest.mark.parametrize("k", [2, 8, 16, 17, 32])
def test_knn_k_sweep_uniform(gpu_ctx, oracle, k):
    xyz = synth.uniform(30000, seed=11)
    _check_knn_normals(gpu_ctx, oracle, xyz, k)


def test_facade_200k_k16(gpu_ctx, oracle):
    xyz = synth.facade(n_side=450, seed=2)
    neigh, normals = _check_knn_normals(gpu_ctx, oracle, xyz, 16)
    _check_grow(gpu_ctx, oracle, xyz, normals, neigh)


def test_segment_fused_matches_stages(gpu_ctx, oracle):
    xyz = synth.urban(150_000, seed=5)
    p = api.default_params(k=16)
    neigh, normals, plane_idx, planes = gpu_ctx.segment(xyz, p)
    oneigh, onormals = oracle.knn_normals(xyz, k=16)
    assert np.array_equal(neigh, oneigh) and np.array_equal(normals, onormals)
    opi, opl = oracle.region_grow(xyz, onormals, oneigh)
    assert np.array_equal(plane_idx, opi)
    assert sum(len(p.pointIdx) for p in planes) == len(opl["point_idx"])


# ---- golden fixtures: the reference's own stage-3 outputs (tests/golden) ----
import glob
import os

GOLD = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz"))
              if not os.path.basename(p).startswith(("raster_", "ply_")))  # stage-3 fixtures (raster / PLY ones have their own tests)


@pytest.mark.parametrize("mode", RG_MODES)
@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_region_grow_matches_reference_golden(gpu_ctx, path, mode):
    _check_golden(gpu_ctx, path, mode)


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_first_step_engine_fallback_matches_reference_golden(gpu_ctx, path, monkeypatch):
    """BS_GROW_V2=0 puts the k <= 16 rounds on the first step engine (grow_spec_kernel<16>), the fallback of the
    default grow_spec2_kernel<16>: the same bits as the reference (the switch is read on every call)."""
    assert np.load(path)["neigh"].shape[1] <= 16
    monkeypatch.setenv("BS_GROW_V2", "0")
    _check_golden(gpu_ctx, path, 2)


def _check_golden(gpu_ctx, path, mode):
    g = np.load(path)
    k = g["neigh"].shape[1]
    pi, planes = gpu_ctx.region_grow(g["xyz"], g["normals"], g["neigh"], api.default_params(k=k, rg_mode=mode))
    assert np.array_equal(pi, g["plane_idx"])
    assert [p.id for p in planes] == g["id"].tolist()
    for i, p in enumerate(planes):
        assert np.array_equal(p.pointIdx, g["point_idx"][g["offset"][i]:g["offset"][i + 1]])
        assert np.array_equal(p.center, g["center"][i])
        assert np.array_equal(p.normal, g["normal"][i])


def test_legacy_adapter_colours_match_reference(gpu_ctx):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "plane_cube_12k.npz"))
    h = api.SegPlane(g["xyz"], g["normals"], g["neigh"], 15, ctx=gpu_ctx)
    planes = h.get_planes()
    assert np.array_equal(h.planeIdx, g["plane_idx"])
    assert np.array_equal(h.set_plane_color(planes), g["colors"])  # glibc rand(), G,B,R slots


# ---- edge cases ----------------------------------------------------------------

def test_duplicates_and_exact_ties(gpu_ctx, oracle):
    rng = np.random.default_rng(5)
    xyz = (rng.integers(0, 12, (5000, 3)) * 25).astype(np.int32)  # heavy duplication, ties everywhere
    neigh, normals = _check_knn_normals(gpu_ctx, oracle, xyz, 15)
    _check_grow(gpu_ctx, oracle, xyz, normals, neigh)


def test_dense_ball_exceeds_max_nn(gpu_ctx, oracle):
    rng = np.random.default_rng(9)
    xyz = rng.integers(0, 150, (6000, 3)).astype(np.int32)  # > 50 points inside every r=100 ball
    _check_knn_normals(gpu_ctx, oracle, xyz, 16)
    assert gpu_ctx.timings()["n_fallback_queries"] > 0


def test_sparse_outliers_need_far_rings(gpu_ctx, oracle):
    a = synth.uniform(4000, seed=4)
    far = np.array([[200000, 5, 5], [5, 300000, 7], [400000, 400000, 400000], [-90000, 0, 0]], np.int32)
    xyz = np.concatenate([a, far]).astype(np.int32)
    _check_knn_normals(gpu_ctx, oracle, xyz, 15)


def test_n_equals_k(gpu_ctx, oracle):
    xyz = synth.uniform(16, seed=8)
    neigh, normals = _check_knn_normals(gpu_ctx, oracle, xyz, 16)
    _check_grow(gpu_ctx, oracle, xyz, normals, neigh)


def test_explicit_cell_size_and_thresholds(gpu_ctx, oracle):
    xyz = synth.plane_cube()[:40000].copy()
    ref = _check_knn_normals(gpu_ctx, oracle, xyz, 15)
    for cell in (60, 333, 9000):  # 9000 mm forces the general kernel for every query
        p = api.default_params(k=15, cell_size=cell)
        ng, nr = gpu_ctx.knn_normals(xyz, p)
        assert np.array_equal(ng, ref[0]) and np.array_equal(nr, ref[1])
    _check_grow(gpu_ctx, oracle, xyz, ref[1], ref[0], th_thickness=40, th_point_count=50, cos_th=0.97)


def test_error_codes(gpu_ctx):
    xyz = synth.uniform(10, seed=1)
    with pytest.raises(api.BsError) as e:
        gpu_ctx.knn_normals(xyz, api.default_params(k=15))  # n < k: the reference is UB here
    assert e.value.status == -1
    with pytest.raises(api.BsError) as e:
        gpu_ctx.knn_normals(synth.uniform(100, seed=1), api.default_params(k=40))
    assert e.value.status == -1
    big = synth.uniform(100, seed=1).copy()
    big[0, 0] = 1 << 24
    with pytest.raises(api.BsError) as e:
        gpu_ctx.knn_normals(big, api.default_params(k=15))
    assert e.value.status == -2
    bad = np.zeros((100, 15), np.int32)
    bad[3, 3] = 100
    with pytest.raises(api.BsError) as e:
        gpu_ctx.region_grow(synth.uniform(100, seed=1), np.tile([0.0, 0.0, 1.0], (100, 1)), bad,
                            api.default_params(k=15))
    assert e.value.status == -1


def test_negative_coordinates_without_shift(gpu_ctx, oracle):
    xyz = synth.plane_cube()[:20000].astype(np.int64) - 4000
    _check_knn_normals(gpu_ctx, oracle, xyz.astype(np.int32), 15)


def test_halo_slab_form_matches_global_result(gpu_ctx, oracle):
    """bs_knn_normals_halo (the per-GPU piece of the sharded path): two Morton
    slabs processed one after the other on this GPU must reproduce the global
    neighbour indices / normals; a thin halo must be reported as uncertified."""
    from buildingsegment_amd import dist as bsd
    xyz = synth.plane_cube()[:30000].copy()
    p = api.default_params(k=15)
    ng, nr = oracle.knn_normals(xyz, k=15)
    for r in range(2):
        own_xyz, own_idx = bsd.partition_morton(xyz, 2, r)
        other = np.setdiff1d(np.arange(len(xyz)), own_idx)
        for h, expect_ok in ((300.0, True), (20.0, False)):
            # halo = every foreign point within h (L-inf) of some own point: brute force via voxels of edge h
            v = int(h)
            own_vox = set(map(tuple, (own_xyz // v)))
            ov = xyz[other] // v
            near = np.array([any((a + dx, b + dy, c + dz) in own_vox for dx in (-1, 0, 1) for dy in (-1, 0, 1)
                                 for dz in (-1, 0, 1)) for a, b, c in ov])
            loc_xyz = np.concatenate([own_xyz, xyz[other][near]]).astype(np.int32)
            loc_idx = np.concatenate([own_idx, other[near].astype(np.int32)]).astype(np.int32)
            neigh, normals, unc = gpu_ctx.knn_normals_halo(loc_xyz, loc_idx, len(own_idx), p, h)
            if expect_ok:
                assert unc == 0
                assert np.array_equal(neigh, ng[own_idx]) and np.array_equal(normals, nr[own_idx])
            else:
                assert unc > 0


# ---- stress of the speculative scheduler (rg_mode 2) against the oracle ------------

def _noisy_walls(n_per, seed, noise, shuffle=True, gap=100, flip=True):
    """Three noisy square walls meeting at a corner.  gap: distance of the second and third wall from the others'
    planes (mm); flip: every normal is turned to z >= 0, which on the two walls whose normal has a NOISE z component
    gives neighbours of opposite sign."""
    rng = np.random.default_rng(seed)
    m = int(np.sqrt(n_per))
    u, v = np.meshgrid(np.arange(m) * 40, np.arange(m) * 40, indexing="ij")
    u = u.ravel() + rng.integers(-10, 11, m * m)
    v = v.ravel() + rng.integers(-10, 11, m * m)
    w = rng.integers(-30, 31, m * m)
    faces = [np.stack([u, v, w], 1), np.stack([u, w, v + gap], 1), np.stack([w, u + gap, v + gap], 1)]
    tn = [np.array([0, 0, 1.0]), np.array([0, 1.0, 0]), np.array([1.0, 0, 0])]
    xyz = np.concatenate(faces).astype(np.int64)
    nrm = np.concatenate([np.tile(t, (m * m, 1)) for t in tn]) + rng.normal(0, noise, (3 * m * m, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    if flip:
        nrm[nrm[:, 2] < 0] *= -1
    if shuffle:
        perm = rng.permutation(len(xyz))
        xyz, nrm = xyz[perm], nrm[perm]
    xyz -= xyz.min(0)
    return xyz.astype(np.int32), np.ascontiguousarray(nrm)


@pytest.mark.parametrize("cfg", [
    dict(n_per=20000, seed=1, noise=0.05, k=15, th_point_count=400),
    dict(n_per=20000, seed=2, noise=0.25, k=15, th_point_count=400),   # orphans dominate
    dict(n_per=12000, seed=3, noise=0.15, k=8, th_point_count=20),     # many tiny planes and roll-backs
    dict(n_per=12000, seed=4, noise=0.10, k=24, th_point_count=0),     # every grown plane commits
    # raster order: deep chains.  Commits NO plane in the oracle (89 787 points, 18 413 attempts; th_point_count 0 gives
    # none either): in this order a seed that fails at depth 0 leaves its labels behind (my_function.cpp:238-239) and
    # so fails the next seed, wall after wall; lower k or lower noise do not change it (k = 6 commits one plane).  It
    # checks the labels of a long cascade of failures, never a plane's list, centre or normal: see the last case.
    dict(n_per=30000, seed=5, noise=0.02, k=16, th_point_count=400, shuffle=False, planes=0),
    dict(n_per=9000, seed=6, noise=0.30, k=4, th_point_count=3, cos_th=0.5),
    # The sibling of the raster-order case above, also in raster order: the walls 2 m apart and their normals not
    # turned to z >= 0 (the turn gives the second and third wall neighbours of opposite sign, which no seed survives
    # in this order).  Every
    # wall's first point seeds a plane that runs through the whole wall: 3 planes of ~29 900 entries.
    dict(n_per=30000, seed=5, noise=0.02, k=16, th_point_count=400, shuffle=False, gap=2000, flip=False, planes=3),
])
def test_speculative_grow_stress(gpu_ctx, oracle, cfg):
    xyz, nrm = _noisy_walls(cfg["n_per"], cfg["seed"], cfg["noise"], cfg.get("shuffle", True), cfg.get("gap", 100),
                            cfg.get("flip", True))
    k = cfg["k"]
    neigh = oracle.knn_normals(xyz, k=k, want_normals=False)[0]
    kw = dict(th_point_count=cfg["th_point_count"])
    if "cos_th" in cfg:
        kw["cos_th"] = cfg["cos_th"]
    plane_idx, planes = _check_grow_mode(gpu_ctx, oracle, xyz, nrm, neigh, 2, **kw)
    if "planes" in cfg:  # (measured with the oracle; the comparison above makes it the oracle's count)
        assert len(planes) == cfg["planes"]


def test_speculative_grow_urban_400k(gpu_ctx, oracle):
    """Many independent faces: the multi-plane path proper (pending planes,
    dead-plane reclaim, several rounds)."""
    xyz = synth.urban(400_000, seed=9)
    neigh, normals = gpu_ctx.knn_normals(xyz, api.default_params(k=16))
    _check_grow_mode(gpu_ctx, oracle, xyz, normals, neigh, 2)
    assert gpu_ctx.timings()["rg_rounds"] >= 1


def test_bench_workload_facade_1m_full_parity(gpu_ctx, oracle):
    """The bench.py N=1 workload (BASELINE.json configs[1]) end to end against
    the oracle: every neighbour index, normal, label and plane list."""
    xyz = synth.facade(n_side=1000, seed=2)
    p = api.default_params(k=16)
    neigh, normals, plane_idx, planes = gpu_ctx.segment(xyz, p)
    oneigh, onormals = oracle.knn_normals(xyz, k=16)
    assert np.array_equal(neigh, oneigh)
    assert np.array_equal(normals, onormals)
    opi, opl = oracle.region_grow(xyz, onormals, oneigh)
    assert np.array_equal(plane_idx, opi)
    assert [len(q.pointIdx) for q in planes] == np.diff(opl["offset"]).tolist()
    assert np.array_equal(np.concatenate([q.pointIdx for q in planes]), opl["point_idx"])
    # size-independent properties at full size
    d = xyz[neigh].astype(np.int64) - xyz[:, None, :].astype(np.int64)
    d2 = (d * d).sum(-1)
    assert (np.diff(d2, axis=1) >= 0).all() and (neigh[:, 0] == np.arange(len(xyz))).all()
    assert np.abs(np.linalg.norm(normals, axis=1) - 1).max() < 1e-12 and (normals[:, 2] >= 0).all()
    labelled = plane_idx[plane_idx > 0]
    assert labelled.max() <= len(planes) + 1 and (plane_idx != 0).all()


def test_device_pre_and_post_processing(gpu_ctx, oracle):
    """SURVEY 8f-2,3: bbox shift (buildingSeg ctor, TMC3.cpp:55-73) and colour
    scatter (set_plane_color, my_function.cpp:260-275) on device-resident buffers."""
    import torch
    raw = synth.plane_cube()[:20000].astype(np.int64) + np.array([5000, -250, 77])
    d_xyz = torch.from_numpy(raw.astype(np.int32)).cuda()
    n = len(raw)
    mn = gpu_ctx.shift_to_origin_dev(d_xyz.data_ptr(), n)
    assert mn.tolist() == raw.min(0).tolist()
    shifted = (raw - raw.min(0)).astype(np.int32)
    assert np.array_equal(d_xyz.cpu().numpy(), shifted)
    p = api.default_params(k=15)
    d_plane = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu_ctx.segment_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), p)
    planes = gpu_ctx.planes_fetch()
    ng, nr = oracle.knn_normals(shifted, k=15)
    opi, opl = oracle.region_grow(shifted, nr, ng)
    assert np.array_equal(d_plane.cpu().numpy(), opi) and len(planes) == len(opl["id"])
    rgb = np.arange(3 * len(planes), dtype=np.int32).reshape(-1, 3) + 60
    d_col = torch.full((n, 3), 999, dtype=torch.int16, device="cuda")
    gpu_ctx.plane_colors_dev(rgb, n, d_col.data_ptr())
    want = np.zeros((n, 3), np.uint16)
    for i, q in enumerate(planes):
        want[q.pointIdx] = rgb[i]
    assert np.array_equal(d_col.cpu().numpy().view(np.uint16), want)


def test_regression_fuzz_7_106_unsettled_claims(gpu_ctx, oracle):
    """Found by tests/tools/fuzz_parity.py: k=4, cos_th=0 on a curved sheet gives ~18 000
    plane attempts (10 commit).  A plane that failed at depth 0 left its optimistic
    claims unsettled, its victim reclaimed the point and held it twice while passing
    validation.  Must be exact, repeatedly, at full concurrency."""
    g = np.load(os.path.join(os.path.dirname(__file__), "data", "fuzz_fail_7_106.npz"))
    p = api.default_params(k=int(g["k"]), th_thickness=int(g["th"]), th_point_count=int(g["cnt"]),
                           cos_th=float(g["cos"]), rg_mode=2)
    opi, opl = oracle.region_grow(g["xyz"], g["normals"], g["neigh"], th_thickness=p.th_thickness,
                                  th_point_count=p.th_point_count, cos_th=p.cos_th)
    for _ in range(3):
        pi, planes = gpu_ctx.region_grow(g["xyz"], g["normals"], g["neigh"], p)
        assert np.array_equal(pi, opi)
        assert [len(q.pointIdx) for q in planes] == np.diff(opl["offset"]).tolist()


def test_first_knn_kernel_is_bit_identical(gpu_ctx, oracle, monkeypatch):
    """BS_KNN_BUFFERED=0 selects the first fast kernel (insertion network per candidate, kept for A/B runs): it must
    produce exactly what the default kernel and the oracle produce."""
    monkeypatch.setenv("BS_KNN_BUFFERED", "0")
    for xyz, k in ((synth.plane_cube()[:60000].copy(), 15), (synth.uniform(40000, seed=21), 32),
                   (synth.urban(120_000, seed=8), 16)):
        _check_knn_normals(gpu_ctx, oracle, xyz, k)


def test_knn_moment_sums_64_bit_and_relative_32_bit_agree(gpu_ctx, oracle, monkeypatch):
    """The default kernel keeps the moment sums relative to the query in 32-bit registers when r <= 181 mm and in 64-bit
    absolute sums otherwise (BS_KNN_MOMENTS64=1 forces the latter): normals must equal the oracle's bit for bit either
    way, also for a cloud far from the origin (large absolute coordinates, the conversion's worst case)."""
    far = synth.urban(100_000, seed=8) + np.array([8_000_000, -8_000_000, 7_500_000], np.int32)
    cases = ((synth.urban(120_000, seed=8), 16, {}), (far, 16, {}), (synth.uniform(40000, seed=21), 32, {}),
             (synth.urban(120_000, seed=8), 16, {"radius": 250.0}), (far, 15, {"radius": 181.0}), (far, 15, {"radius": 182.0}))
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("BS_KNN_MOMENTS64", env)
        else:
            monkeypatch.delenv("BS_KNN_MOMENTS64", raising=False)
        for xyz, k, kw in cases:
            _check_knn_normals(gpu_ctx, oracle, xyz, k, **kw)


def test_general_knn_by_the_wave_and_by_the_thread_agree(gpu_ctx, oracle, monkeypatch):
    """Work-listed queries (more than max_nn points inside the radius, or uncertified within the fast kernel's rings) go to
    knn_general_wave_kernel and from there -- buffer overflow, still uncertified -- to the one-thread kernel.  Dense
    blobs (max_nn 3..50 inside a radius that holds hundreds), a sparse cloud whose rings run out (full scan) and
    BS_KNN_GENERAL_THREAD=1 (the one-thread kernel alone) must all equal the oracle, with the same work list."""
    rng = np.random.default_rng(77)
    dense = rng.integers(0, 600, (30000, 3)).astype(np.int32)  # ~580 points inside r = 100: every query is work-listed
    lattice = (rng.integers(0, 12, (20000, 3)) * 40).astype(np.int32)  # duplicates and exact ties, > GCAP candidates per ring
    sparse = np.concatenate([rng.integers(0, 2000, (3000, 3)), rng.integers(0, 2000, (40, 3)) + 400000]).astype(np.int32)
    counts = {}
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("BS_KNN_GENERAL_THREAD", env)
        else:
            monkeypatch.delenv("BS_KNN_GENERAL_THREAD", raising=False)
        for name, xyz, k, kw in (("dense", dense, 16, {}), ("dense_small_m", dense, 8, {"max_nn": 5}), ("lattice", lattice, 32, {}),
                                 ("sparse", sparse, 15, {}), ("uniform", synth.uniform(60000, seed=5), 16, {})):
            _check_knn_normals(gpu_ctx, oracle, xyz, k, **kw)
            counts.setdefault(name, set()).add(gpu_ctx.timings()["n_fallback_queries"])
    assert all(len(v) == 1 for v in counts.values()), counts
    assert min(counts["dense"]) > 20000 and min(counts["sparse"]) > 0


@pytest.mark.gpu
def test_center_div_device_exact(gpu_ctx):
    """csrc/bs_centerdiv.h on the device (hardware reciprocal seed + one Newton
    step + one integer correction) against the reference expression
    (int32)((uint64)(int64)c / n) of my_function.cpp:249-250: edge values, every
    small n, and 8 M random pairs.  Bit-exact."""
    rng = np.random.default_rng(99)
    cs = np.array([0, 1, -1, 2, -2, 2**31 - 1, -2**31, -2**31 + 1, 1000, -1000, 65536, -65536], dtype=np.int64)
    ns = np.array([1, 2, 3, 4, 5, 7, 255, 256, 257, 65535, 65536, 65537, 10**6, 2**31 - 1, 2**31 - 2, 2**30, 2**30 - 1,
                   3000, 108197], dtype=np.int64)
    c0, n0 = [a.ravel() for a in np.meshgrid(cs, ns)]
    n1 = np.repeat(np.arange(1, 4000, dtype=np.int64), 6)
    c1 = np.tile(np.array([2**31 - 1, -2**31, -1, -7, 123456789, -123456789], dtype=np.int64), 3999)
    m = 8_000_000
    c2 = rng.integers(-2**31, 2**31, m)
    kind = rng.integers(0, 4, m)
    n2 = np.where(kind == 0, rng.integers(1, 1000, m),
                  np.where(kind == 1, rng.integers(1, 200000, m),
                           np.where(kind == 2, rng.integers(1, 2**31 - 1, m), 1 << rng.integers(0, 31, m))))
    c = np.concatenate([c0, c1, c2]).astype(np.int32)
    n = np.concatenate([n0, n1, n2]).astype(np.uint32)
    got = gpu_ctx.selftest_center_div(c, n)
    ref = ((c.astype(np.int64).view(np.uint64)) // n.astype(np.uint64)).astype(np.uint32).view(np.int32)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (c[bad[:5]], n[bad[:5]], got[bad[:5]], ref[bad[:5]])


@pytest.mark.gpu
def test_fuzz_negative_coordinates_and_noisy_normals():
    """40 differential fuzz cases (tests/tools/fuzz_parity.py: negative coordinates,
    perturbed non-unit normals, tiny planes, both grow modes).  Plane normals and
    centres are part of the comparison: an inexact plane-centre division that
    still produced the right labels was caught by exactly these cases."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "tools", "fuzz_parity.py"), "--cases", "40", "--seed", "4242", "--audit"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "40 cases, 0 mismatches" in out.stdout


@pytest.mark.gpu
def test_regression_fuzz_2718_16_reclaim_aba():
    """Fuzz case 2718/16 (29 k points, thickness 2000, min plane size 0: many small adjacent
    planes that kill and re-grow each other inside one launch).  A later plane used to reclaim
    a point from a plane whose dead flag it had read just before that plane came back to life
    and claimed the same point again under the same tag; the live plane then took the point back
    and held it twice.  The result passed validation with duplicated list entries and a wrong
    normal/centre in ~35 % of the runs; labels were still right.  25 repetitions of the growth."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "tools", "fuzz_parity.py"), "--cases", "17", "--seed", "2718",
                          "--only", "16", "--repeat", "25"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "0 mismatches" in out.stdout


@pytest.mark.parametrize("mode", [1, 2])
def test_validation_rejects_a_forged_plane(gpu_ctx, oracle, mode):
    """The post-round validation is a certificate, not a smoke test: a finished plane whose list holds a point
    twice (mode 1) or whose reported normal differs from the sum over its list by one ulp (mode 2) -- the
    signatures of the claim-protocol bugs found by fuzzing in round 1 -- must be refused (validate1 /
    validate3 in bs_grow_spec.hip), grown again, and the final result must still equal the oracle's.
    (my_function.cpp:226-233,241-250)"""
    from buildingsegment_amd import api, synth
    xyz = synth.plane_cube()[:40000].copy()
    neigh, normals = oracle.knn_normals(xyz, k=15)
    opi, opl = oracle.region_grow(xyz, normals, neigh)
    p = api.default_params(k=15)
    gpu_ctx.region_grow(xyz, normals, neigh, p)
    assert gpu_ctx.timings()["forged_seed"] == -1 and gpu_ctx.timings()["forged_refused"] == 0
    rounds_clean = gpu_ctx.timings()["rg_rounds"]
    gpu_ctx.selftest_forge_next(mode)
    pi, planes = gpu_ctx.region_grow(xyz, normals, neigh, p)
    tm = gpu_ctx.timings()
    assert tm["forged_seed"] >= 0, "no plane was forged"
    assert tm["forged_refused"] == 1 and tm["validation_rejects"] >= 1, "the forged plane passed the validation"
    assert tm["rg_rounds"] > rounds_clean  # ... and was grown again
    assert np.array_equal(pi, opi) and len(planes) == len(opl["id"])
    assert np.array_equal(np.concatenate([q.pointIdx for q in planes]), opl["point_idx"])
    assert np.array_equal(np.stack([q.normal for q in planes]), opl["normal"])
    assert np.array_equal(np.stack([q.center for q in planes]), opl["center"])
    gpu_ctx.region_grow(xyz, normals, neigh, p)  # the hook is one-shot
    assert gpu_ctx.timings()["forged_seed"] == -1


def test_audit_replays_every_plane_attempt(gpu_ctx, oracle):
    """bs_set_audit: after the speculative grow, every plane attempt that exists under the final owners is grown
    again WITHOUT speculation (owner below the seed = taken, everything else free at the seed's time) and must
    reproduce the committed list entry by entry, normal and centre bit for bit; attempts that were not committed
    must end at or below the commit threshold.  The number of attempts found that way equals the number the
    speculative rounds finalised.  (my_function.cpp:180-258)"""
    from buildingsegment_amd import api, synth
    gpu_ctx.set_audit(True)
    try:
        for xyz, k in ((synth.plane_cube(), 15), (synth.facade(400, seed=9), 16), (synth.urban(300_000, seed=8), 16),
                       (synth.uniform(20_000, seed=3), 8)):
            xyz = np.ascontiguousarray(xyz)
            neigh, normals, plane_idx, planes = gpu_ctx.segment(xyz, api.default_params(k=k))
            tm = gpu_ctx.timings()
            assert tm["audit_attempts"] == tm["n_seed_attempts"] >= len(planes), tm
            assert tm["audit_mismatches"] == 0, tm
    finally:
        gpu_ctx.set_audit(False)
    gpu_ctx.segment(np.ascontiguousarray(synth.plane_cube()), api.default_params(k=15))
    assert gpu_ctx.timings()["audit_attempts"] == -1  # off again


AUDIT_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from buildingsegment_amd import api, synth
ctx = api.Context(0)
ctx.set_audit(True)
xyz = np.ascontiguousarray(synth.plane_cube()[:40000])
p = api.default_params(k=15)
ctx.segment(xyz, p)
clean = ctx.timings()
ctx.selftest_forge_next(2)
ctx.segment(xyz, p)
tm = ctx.timings()
print("RESULT", clean["audit_mismatches"], tm["forged_seed"], tm["forged_refused"], tm["audit_mismatches"])
"""


def test_audit_catches_what_a_disabled_validator_lets_through():
    """With validate3 switched off (developer switch BS_NO_VALIDATE3) a plane whose reported normal was forged by
    one ulp is committed; the audit's replay must flag it."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BS_NO_VALIDATE3="1")
    out = subprocess.run([sys.executable, "-c", AUDIT_CHILD, root], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][0].split()
    clean_mis, forged_seed, forged_refused, mis = (int(v) for v in line[1:])
    assert clean_mis == 0
    assert forged_seed >= 0 and forged_refused == 0, "the forgery did not get past the (disabled) validator"
    assert mis >= 1, "the audit did not notice the forged plane"


def test_region_grow_after_segment_does_not_reuse_the_fused_scratch(gpu_ctx, oracle):
    """bs_segment keeps position-ordered copies of its k-lists and normals for the grower, keyed by buffer
    pointers.  A later bs_region_grow on the same context -- same n, same k, same staging buffers, DIFFERENT
    neighbour lists and normals -- must not see them."""
    from buildingsegment_amd import api, synth
    a = np.ascontiguousarray(synth.plane_cube()[:20000])
    b = np.ascontiguousarray(synth.urban(60_000, seed=21)[:20000])
    p = api.default_params(k=15)
    gpu_ctx.segment(a, p)
    neigh, normals = oracle.knn_normals(b, k=15)
    rng = np.random.default_rng(5)
    nrm = normals + rng.normal(0, 0.05, normals.shape)
    nrm = np.ascontiguousarray(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    opi, opl = oracle.region_grow(b, nrm, neigh)
    pi, planes = gpu_ctx.region_grow(b, nrm, neigh, p)
    assert np.array_equal(pi, opi) and len(planes) == len(opl["id"])
    if planes:
        assert np.array_equal(np.concatenate([q.pointIdx for q in planes]), opl["point_idx"])


@pytest.mark.parametrize("rg_mode", [0, 1])
def test_rows_with_repeated_indices_match_the_reference_semantics(gpu_ctx, oracle, rg_mode):
    """Caller-supplied k-lists may repeat an index in slots 1..K-1 (bs_region_grow takes any rows).  The reference
    labels a point on first sight and skips it on the second (my_function.cpp:226-233); a seed with a repeat never
    reaches K-1 accepted neighbours (:238).  The HIP path must do the same (the fast claim path let both
    lanes push)."""
    from buildingsegment_amd import api, synth
    xyz = synth.boxes(n_boxes=2, seed=33)
    ng, nr = oracle.knn_normals(xyz, k=15)
    rng = np.random.default_rng(9)
    ng = ng.copy()
    rows = rng.choice(len(xyz), size=len(xyz) // 12, replace=False)
    dst = rng.integers(2, 15, size=len(rows))
    src = np.array([rng.integers(1, d) for d in dst])
    ng[rows, dst] = ng[rows, src]  # slot dst repeats slot src (1 <= src < dst)
    opi, opl = oracle.region_grow(xyz, nr, ng)
    pi, planes = gpu_ctx.region_grow(xyz, nr, ng, api.default_params(k=15, rg_mode=rg_mode))
    assert np.array_equal(pi, opi)
    assert len(planes) == len(opl["id"])
    off = opl["offset"]
    for i, pl in enumerate(planes):
        assert np.array_equal(pl.pointIdx, opl["point_idx"][off[i]:off[i + 1]])
        assert np.array_equal(pl.center, opl["center"][i])
        assert np.array_equal(pl.normal.view(np.int64), opl["normal"][i].view(np.int64))
    assert (pi > 0).sum() > 1000 and len(planes) >= 1  # the planes still grow around the crippled seeds
