"""N>1 path on CPU: world_size-2/3/5 gloo runs of buildingsegment_amd.dist.segment_sharded_dev
with the CPU oracle injected as compute backend (the HIP backend needs a GPU).  The
orchestration under test is the SAME code bench.py --gpus N runs on device tensors: Morton
partition (all-to-all), voxel halo (all-to-all), certification + retry, distributed
union-find (all-reduce MIN), component deal + redistribution (all-to-all), per-rank region
growing of whole components, global plane ids from the all-gathered committed seeds, label
all-reduce; plus the agreement on failures (no rank may be left waiting in a collective)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "shard_ref"))
import scenarios as S  # noqa: E402


class OracleBackend:
    """CPU restatement of the backend contract of buildingsegment_amd.dist (see its docstring).
    Slab kNN: ties by GLOBAL index (local cloud sorted by gidx first), global indices out,
    certification = k-th distance < cert_radius."""

    def __init__(self, fail_grow_on_rank=None):
        from oracle import oracle as O
        self.O = O
        self.fail_grow_on_rank = fail_grow_on_rank

    def knn_normals(self, xyz_loc, gidx_loc, n_query, params, cert_radius):
        xyz_local, gidx = xyz_loc.numpy(), gidx_loc.numpy()
        order = np.argsort(gidx, kind="stable")
        rank_of = np.empty(len(order), np.int64)
        rank_of[order] = np.arange(len(order))
        xs, gs = np.ascontiguousarray(xyz_local[order]), gidx[order]
        ng, nr = self.O.knn_normals(xs, k=params.k, radius=params.radius, max_nn=params.max_nn)
        q = rank_of[:n_query]
        ngq, nrq = ng[q], nr[q]
        unc = 0
        if cert_radius > 0:
            d = xs[ngq[:, -1]].astype(np.int64) - xs[q].astype(np.int64)
            unc = int(((d * d).sum(1) >= cert_radius * cert_radius).sum())
        return torch.from_numpy(gs[ngq].astype(np.int32)), torch.from_numpy(nrq), unc

    def cc_hook(self, rows, gidx, parent):
        """bs_cc_hook_dev restated with numpy (vectorised hooking + pointer jumping)."""
        P = parent.numpy()  # shares the tensor's memory: updated in place
        u = np.repeat(gidx.numpy().astype(np.int64), rows.shape[1])
        v = rows.numpy().reshape(-1).astype(np.int64)

        def find(x):
            r = P[x].astype(np.int64)
            while True:
                rr = P[r].astype(np.int64)
                if (rr == r).all():
                    return r
                r = rr

        hooks = 0
        while True:
            ru, rv = find(u), find(v)
            m = ru != rv
            if not m.any():
                break
            hi, lo = np.maximum(ru[m], rv[m]), np.minimum(ru[m], rv[m])
            np.minimum.at(P, hi, lo.astype(P.dtype))
            hooks += len(np.unique(hi))
        touched = np.unique(np.concatenate([u, v]))
        P[touched] = find(touched).astype(P.dtype)
        return hooks

    def remap_rows(self, rows, sorted_gidx):
        sg, r = sorted_gidx.numpy(), rows.numpy()
        pos = np.searchsorted(sg, r)
        ok = (pos < len(sg)) & (sg[np.minimum(pos, len(sg) - 1)] == r)
        return torch.from_numpy(np.where(ok, pos, 0).astype(np.int32)), int((~ok).any())

    def region_grow(self, xyz, normals, neigh, params):
        if self.fail_grow_on_rank is not None and dist.get_rank() == self.fail_grow_on_rank:
            raise RuntimeError("injected failure")
        pi, pl, ow = self.O.region_grow(xyz.numpy(), normals.numpy(), neigh.numpy(), th_thickness=params.th_thickness,
                                        th_point_count=params.th_point_count, cos_th=params.cos_th, want_owner=True)
        seeds = pl["point_idx"][pl["offset"][:-1]].astype(np.int32)
        return torch.from_numpy(pi), torch.from_numpy(ow), torch.from_numpy(seeds), (lambda: pl)

    def labels_from_owner(self, owner, seeds):
        o, s = owner.numpy(), seeds.numpy()
        return torch.from_numpy(np.where(o >= 0, 1 + np.searchsorted(s, o, side="left"), -1).astype(np.int32))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _params(k=15):
    from buildingsegment_amd import _lib
    return _lib.Params(k=k, max_nn=50, radius=100.0, th_thickness=300, th_point_count=400, cos_th=0.88,
                       cell_size=0, rg_mode=0)


def _cloud(name):
    from buildingsegment_amd import synth
    if name in S.BY_NAME:  # a cloud of the scenario table (tests/shard_ref/scenarios.py)
        return np.array(S.cloud(S.BY_NAME[name]))
    return synth.plane_cube()[:24000].copy() if name == "plane_cube" else synth.boxes()


def _worker(rank, world, port, halo, out, cloud, fail_rank, rule=None):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from buildingsegment_amd import dist as bsd
    xyz = _cloud(cloud)
    n = len(xyz)
    b = bsd.slab_bounds(n, world)  # the input split is arbitrary: a contiguous 1/N of the input order
    d_xyz = torch.from_numpy(xyz[b[rank]:b[rank + 1]])
    d_gidx = torch.arange(b[rank], b[rank + 1], dtype=torch.int32)
    if rule is not None:  # ... or any other 1/N: a share rule of the scenario table
        idx = S.shares(rule, n, world)[rank]
        d_xyz, d_gidx = torch.from_numpy(np.ascontiguousarray(xyz[idx])), torch.from_numpy(idx.copy())
    try:
        labels, info = bsd.segment_sharded_dev(OracleBackend(fail_rank), d_xyz, d_gidx, n, _params(), halo=halo, want_planes=True)
    except bsd.ShardError as e:
        open(out % rank + ".err", "w").write(str(e))
        dist.destroy_process_group()
        return
    planes = bsd.gather_planes(info["planes"])
    np.savez(out % rank, idx=info["gidx_own"].numpy(), ng=info["neigh_own"].numpy(), nr=info["normals_own"].numpy(),
             labels=labels.numpy(), retries=info["retries"], n_local=info["n_local"], n_grow=info["n_grow"],
             components=info["components"], cc_iterations=info["cc_iterations"],
             pid=np.array([p["id"] for p in planes], np.int32),
             pnormal=np.array([p["normal"] for p in planes], np.float64).reshape(-1, 3),
             pcenter=np.array([p["center"] for p in planes], np.int32).reshape(-1, 3),
             poff=np.cumsum([0] + [len(p["pointIdx"]) for p in planes]),
             pidx=np.concatenate([p["pointIdx"] for p in planes]) if planes else np.zeros(0, np.int32))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,halo,cloud", [(2, 250.0, "plane_cube"), (2, 30.0, "plane_cube"), (3, 200.0, "boxes"),
                                              (2, 250.0, "boxes"), (5, 150.0, "boxes")])
def test_sharded_run_equals_single_process(oracle, tmp_path, world, halo, cloud):
    out = str(tmp_path / "r%d.npz")
    mp.spawn(_worker, args=(world, _free_port(), halo, out, cloud, None), nprocs=world, join=True)
    xyz = _cloud(cloud)
    ng, nr = oracle.knn_normals(xyz, k=15)
    pi, pl = oracle.region_grow(xyz, nr, ng)
    seen = np.zeros(len(xyz), int)
    sizes, grown = [], []
    for r in range(world):
        g = np.load(out % r)
        assert np.array_equal(g["ng"], ng[g["idx"]])      # neighbour indices bit-exact
        assert np.array_equal(g["nr"], nr[g["idx"]])      # normals bit-exact
        assert np.array_equal(g["labels"], pi)            # labels identical on every rank, equal to the sequential scan
        assert g["n_local"] < len(xyz)                    # a slab + halo, not the whole cloud
        # plane records (gathered): ids, lists (order and duplicates), centres and normals bit for bit
        assert np.array_equal(g["pid"], pl["id"])
        assert np.array_equal(g["poff"], pl["offset"]) and np.array_equal(g["pidx"], pl["point_idx"])
        assert np.array_equal(g["pcenter"], pl["center"])
        assert np.array_equal(g["pnormal"].view(np.int64), pl["normal"].view(np.int64))
        seen[g["idx"]] += 1
        sizes.append(len(g["idx"]))
        grown.append(int(g["n_grow"]))
        if halo < 100:
            assert g["retries"] >= 1                      # halo below the hybrid radius is widened
    assert (seen == 1).all()                              # the Morton slabs partition the cloud
    assert max(sizes) < 1.25 * len(xyz) / world           # ... into nearly equal counts
    assert sum(grown) == len(xyz)                         # stage 3: every point grown by exactly one rank
    if cloud == "boxes":
        assert int(g["components"]) == 6 and sum(1 for v in grown if v > 0) >= min(world, 2)  # the boxes are spread


def _dist_start_halo(halo, radius):
    """the starting halo of dist.segment_sharded_dev, restated: halo if halo > 0 else 2 * radius, at least radius"""
    h = float(halo) if halo > 0 else 2.0 * radius
    return max(h, radius)


@pytest.mark.parametrize("name,world,rule", [("boxes3_contiguous_w2", 3, "interleaved"), ("boxes3_contiguous_w2", 2, "random"),
                                             ("disc_retry1_w3", 3, "random"), ("tiny40_w3", 3, "interleaved")])
def test_scenario_table_through_the_python_orchestration(oracle, tmp_path, name, world, rule):
    """Share rules that are no index ranges, one component across every slab (all of it grows on one rank) and the
    cloud whose slabs cannot fill a k-list, through dist.segment_sharded_dev with k = 15.  The retry count follows from
    the oracle's largest k-th distance and dist.py's own starting halo."""
    import dataclasses
    sc = dataclasses.replace(S.BY_NAME[name], k=15)
    f = S.facts(oracle, sc)
    xyz, n = f["xyz"], len(f["xyz"])
    h0 = _dist_start_halo(sc.halo, _params().radius)
    assert S.retry_margin(f["max_kth"], h0) > 1.0
    retries = S.expected_retries(f["max_kth"], h0)
    out = str(tmp_path / "r%d.npz")
    mp.spawn(_worker, args=(world, _free_port(), sc.halo, out, name, None, rule), nprocs=world, join=True)
    pl = f["planes"]
    seen = np.zeros(n, int)
    grown = []
    for r in range(world):
        g = np.load(out % r)
        assert np.array_equal(g["ng"], f["neigh"][g["idx"]]) and np.array_equal(g["nr"], f["normals"][g["idx"]])
        assert np.array_equal(g["labels"], f["labels"])
        assert np.array_equal(g["pid"], pl["id"])
        assert np.array_equal(g["poff"], pl["offset"]) and np.array_equal(g["pidx"], pl["point_idx"])
        assert np.array_equal(g["pcenter"], pl["center"])
        assert np.array_equal(g["pnormal"].view(np.int64), pl["normal"].view(np.int64))
        assert int(g["retries"]) == retries and int(g["components"]) == f["components"]
        seen[g["idx"]] += 1
        grown.append(int(g["n_grow"]))
    assert (seen == 1).all() and sum(grown) == n
    if f["components"] == 1:
        assert sorted(grown) == [0] * (world - 1) + [n] and int(g["cc_iterations"]) >= 2


def test_failure_on_one_rank_is_raised_on_every_rank(tmp_path):
    """A compute failure on rank 0 (here: injected into region growing) must not leave the other ranks waiting in
    the next collective: all of them raise ShardError."""
    world = 2
    out = str(tmp_path / "r%d.npz")
    mp.spawn(_worker, args=(world, _free_port(), 250.0, out, "boxes", 0), nprocs=world, join=True)
    msgs = [open(out % r + ".err").read() for r in range(world)]
    assert "injected failure" in msgs[0] and "another rank failed in region growing" in msgs[1]


def test_component_deal_is_balanced_and_prefers_home():
    from buildingsegment_amd import dist as bsd
    # 4 components of 100 points on ranks {0: c0 + c1, 1: c2 + half of c3, 2: half of c3}; 1 component split 50 / 50
    roots = np.array([10, 20, 30, 40, 40])
    counts = np.array([100, 100, 100, 60, 40])
    ranks = np.array([0, 0, 1, 1, 2])
    uniq, dest = bsd.assign_components(roots, counts, ranks, 3)
    load = np.bincount(dest, weights=[100, 100, 100, 100], minlength=3)
    assert uniq.tolist() == [10, 20, 30, 40]
    assert load.max() <= 200 and dest[0] == 0  # the first component stays at home; nobody holds more than two
    assert np.array_equal(dest, bsd.assign_components(roots[::-1], counts[::-1], ranks[::-1], 3)[1])  # order-independent
    # one giant component: it stays where most of it is, whatever the balance
    uniq, dest = bsd.assign_components(np.array([7, 7]), np.array([10, 990]), np.array([0, 1]), 2)
    assert dest.tolist() == [1]


def test_single_process_path_without_process_group(oracle):
    """world 1 (no process group): the same function degenerates to the plain pipeline."""
    from buildingsegment_amd import dist as bsd, synth
    xyz = synth.plane_cube()[:9000].copy()
    labels, info = bsd.segment_sharded_dev(OracleBackend(), torch.from_numpy(xyz), torch.arange(len(xyz), dtype=torch.int32),
                                           len(xyz), _params())
    ng, nr = oracle.knn_normals(xyz, k=15)
    pi, _ = oracle.region_grow(xyz, nr, ng)
    assert np.array_equal(info["neigh_own"].numpy(), ng) and np.array_equal(labels.numpy(), pi)


def test_morton_partition_is_a_partition():
    from buildingsegment_amd import dist as bsd, synth
    xyz = synth.uniform(5000, seed=3)
    parts = [bsd.partition_morton(xyz, 4, r)[1] for r in range(4)]
    allidx = np.sort(np.concatenate(parts))
    assert np.array_equal(allidx, np.arange(5000))
    assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
    k = bsd.morton_keys(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.int32))
    assert k.tolist() == [0, 1, 2, 4, 7]


def test_splitter_sample_positions_stay_in_range_beyond_2_pow_24():
    """The slab splitters are sampled at evenly spaced positions of the sorted keys; computed in float32 the last
    position was m (one past the end) as soon as a rank held more than 2^24 points -- bench.py --gpus 2 on the 50 M
    cloud died with a device-side assertion."""
    import torch
    from buildingsegment_amd import dist as D
    for m in (1, 2, 1000, (1 << 24) - 1, (1 << 24) + 1, 25_000_000, 50_000_000, (1 << 31) - 2):
        for samples in (1, 2, 1024):
            pos = D._sample_positions(m, samples, torch.device("cpu"))
            assert pos.dtype == torch.int64 and len(pos) == samples
            assert int(pos.min()) == 0 and int(pos.max()) <= m - 1
            if samples > 1:
                assert int(pos[-1]) == m - 1 and bool((pos[1:] >= pos[:-1]).all())


def _a2a_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    from buildingsegment_amd import dist as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rng = np.random.default_rng(100 + rank)
        ok = True
        for cols, counts in ((16, [0, 1, 7]), (4, [300, 0, 2]), (3, [5, 1000, 33]), (16, [0, 0, 0])):
            counts = counts[rank:] + counts[:rank]  # different per rank
            rows = torch.from_numpy(rng.integers(0, 1 << 30, (sum(counts), cols)).astype(np.int32))
            sc = torch.tensor(counts, dtype=torch.int64)
            D.A2A_MAX_BYTES = 1 << 30
            want, wr = D.all_to_all_rows(rows, sc)
            for limit in (cols * 4, cols * 4 * 7, 100):  # one row per call, seven rows, a limit that is no multiple of a row
                D.A2A_MAX_BYTES = limit
                got, gr = D.all_to_all_rows(rows, sc)
                ok = ok and gr == wr and bool(torch.equal(got, want))
        np.save(os.path.join(out, f"a2a_{rank}.npy"), np.array([1 if ok else 0]))
    finally:
        dist.destroy_process_group()


def test_all_to_all_rows_in_parts_equals_one_call(tmp_path):
    """all_to_all_rows cuts every (source, destination) block into parts when a block exceeds A2A_MAX_BYTES (a 3.2 GB
    payload came back incomplete from one all_to_all_single over RCCL): with tiny limits on three gloo ranks the
    result must equal the single call's, for uneven and empty blocks."""
    import torch.multiprocessing as mp
    world = 3
    mp.spawn(_a2a_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        assert int(np.load(os.path.join(str(tmp_path), f"a2a_{r}.npy"))[0]) == 1
