"""bs_segment_sharded through every branch of its C++ orchestration (csrc/bs_sharded.hip) that one GPU can reach: the
scenarios of tests/shard_ref/scenarios.py, run with thread-ranks on bs_comm_local_create (world 2, 3 and 4) and compared
with the one-process CPU oracle with `==`: labels on every rank, the union of the ranks' plane records (id, pointIdx,
centre, the normal's 64-bit pattern), and the figures of bs_shard_info against the premises that
tests/test_shard_scenarios_cpu.py asserts for the same clouds.

The four contexts of the module are shared by all tests (with the session's: five), so every call also runs on scratch
buffers that an earlier, larger or smaller, call left behind.  BS_COMM_LOCAL_TIMEOUT_S is 60 s in every test and the
threads are joined for 90 s: a mistake in a scenario is a failed test within a minute, not a stuck process."""
import ctypes as C
import os
import sys
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "shard_ref"))
import scenarios as S  # noqa: E402
import thread_ranks as T  # noqa: E402

BS_ERR_INVALID, BS_ERR_INTERNAL, BS_ERR_UNCERTIFIED = -1, -6, -7
GOOD = [sc for sc in S.SCENARIOS if sc.retries is not None]
SAME_ON_EVERY_RANK = ("components", "planes_total", "halo_retries", "halo_mm", "cc_iterations")


@pytest.fixture(autouse=True)
def _deadline(monkeypatch):
    monkeypatch.setenv("BS_COMM_LOCAL_TIMEOUT_S", str(T.COMM_TIMEOUT_S))


@pytest.fixture(scope="module")
def ctxs(gpu_ctx):
    from buildingsegment_amd import api
    cs = [api.Context(0) for _ in range(4)]
    yield cs
    for c in cs:
        c.close()


def _params(sc):
    from buildingsegment_amd import api
    return api.default_params(k=sc.k, rg_mode=sc.rg_mode)


def _run(ctxs, comm, sc, oracle):
    f = S.facts(oracle, sc)
    parts = S.shares(sc.rule, len(f["xyz"]), sc.world)
    return f, parts, T.run_ranks(ctxs[:sc.world], comm, f["xyz"], parts, _params(sc), sc.halo)


def _check(res, f, sc, parts=None):
    """Everything that holds for every scenario -> the info of rank 0."""
    for r, x in enumerate(res):
        assert not isinstance(x, Exception), f"rank {r}: {x}"
    n = len(f["xyz"])
    info0 = res[0][1]
    planes, seen_comps = [], []
    for r, (lab, info, pls) in enumerate(res):
        assert np.array_equal(lab, f["labels"]), f"rank {r}: {(lab != f['labels']).sum()} labels differ"
        for key in SAME_ON_EVERY_RANK:
            assert info[key] == info0[key], (r, key)
        if info["n_grow"] == 0:  # a rank that grew nothing: whole labels (above), no planes
            assert pls == []
        planes += pls
        # component placement: the points of this rank's planes belong to components no other rank has planes of
        comps = set(np.unique(f["comp"][np.concatenate([q.pointIdx for q in pls])]).tolist()) if pls else set()
        assert all(comps.isdisjoint(c) for c in seen_comps)
        seen_comps.append(comps)
    assert sum(x[1]["n_own"] for x in res) == n and sum(x[1]["n_grow"] for x in res) == n
    if parts is None:
        parts = S.shares(sc.rule, n, sc.world)
    # the Morton slabs are those of the partition restated on the CPU (samples, splitters, shift)
    slabs = S.expected_slabs(f["xyz"], parts)
    assert [x[1]["n_own"] for x in res] == [len(s) for s in slabs]
    # ... and every component grows on the rank the deal gives it to: point counts, and the planes by their seeds
    grower, n_grow = S.expected_deal(f["comp"], slabs)
    assert [x[1]["n_grow"] for x in res] == n_grow
    for r, x in enumerate(res):
        assert all(grower[q.pointIdx[0]] == r for q in x[2]), f"rank {r} holds a plane of another rank's component"
    T.check_planes(planes, f["planes"])  # every plane exactly once
    assert info0["planes_total"] == len(f["planes"]["id"])
    assert info0["components"] == f["components"]
    assert info0["halo_retries"] == f["retries"]
    assert info0["halo_mm"] == f["halo_mm"] == f["h0"] * 2 ** f["retries"]
    assert info0["cc_iterations"] >= 2  # hooked and all-reduced, then verified
    idle = sum(1 for x in res if x[1]["n_grow"] == 0)
    assert idle >= sc.world - f["components"]
    print(f"\n[{sc.name}] n={n} " + " ".join(f"{key}={info0[key]}" for key in SAME_ON_EVERY_RANK)
          + " n_own=" + str([x[1]["n_own"] for x in res]) + " n_local=" + str([x[1]["n_local"] for x in res])
          + " n_grow=" + str([x[1]["n_grow"] for x in res]) + " planes=" + str([len(x[2]) for x in res]))
    return info0


@pytest.mark.parametrize("sc", GOOD, ids=[sc.name for sc in GOOD])
def test_scenario_equals_the_oracle(oracle, ctxs, sc):
    comm = T.Comm(sc.world)
    try:
        f, parts, res = _run(ctxs, comm, sc, oracle)
    finally:
        comm.close()
    _check(res, f, sc, parts)
    n = len(f["xyz"])
    if sc.world > f["components"]:  # more ranks than components, or one component for the whole cloud
        idle = [x for x in res if x[1]["n_grow"] == 0]
        assert len(idle) >= sc.world - f["components"] and all(x[2] == [] for x in idle)
    if f["components"] == 1:  # all of it moved to one rank, although every slab border cut k-lists
        assert sorted(x[1]["n_grow"] for x in res) == [0] * (sc.world - 1) + [n]
        assert sum(1 for x in res if x[1]["n_own"] > 0) >= 2
    if sc.rule in ("rank1_nothing", "rank0_everything"):
        assert any(len(p) == 0 for p in parts)  # accepted with d_xyz = d_gidx = 0
        assert all(x[1]["n_own"] > 0 for x in res)  # ... and the partition gave that rank its slab
    if sc.name == "tiny40_w3":
        assert all(x[1]["n_own"] < sc.k for x in res)  # no slab can fill a k-list of its own


def test_no_communicator_at_world_one_equals_segment(oracle, ctxs, gpu_ctx):
    """comm == NULL: no collective is issued.  bs_segment_sharded returns no rows and normals of its own: those of
    ctx.segment are compared with the oracle's, the labels and planes of the two calls with each other."""
    import torch
    sc = S.BY_NAME["boxes3_contiguous_w2"]
    f = S.facts(oracle, sc)
    xyz, n = f["xyz"], len(f["xyz"])
    p = _params(sc)
    neigh, normals, plane_idx, planes = gpu_ctx.segment(xyz, p)
    assert np.array_equal(neigh, f["neigh"]) and np.array_equal(normals.view(np.int64), f["normals"].view(np.int64))
    dev = torch.device("cuda", 0)
    d_xyz = torch.from_numpy(np.array(xyz)).to(dev)
    d_lab = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for d_g in (None, torch.arange(n, dtype=torch.int32, device=dev)):  # identity indices may be NULL at world 1
        torch.cuda.synchronize()
        info = ctxs[0].segment_sharded(None, d_xyz.data_ptr(), d_g.data_ptr() if d_g is not None else 0, n, n,
                                       d_lab.data_ptr(), p, halo=sc.halo)
        lab, pls = d_lab.cpu().numpy(), ctxs[0].sharded_planes_fetch()
        assert np.array_equal(lab, plane_idx) and np.array_equal(lab, f["labels"])
        assert [q.id for q in pls] == [q.id for q in planes]
        for a, b in zip(pls, planes):
            assert np.array_equal(a.pointIdx, b.pointIdx) and np.array_equal(a.center, b.center)
            assert np.array_equal(a.normal.view(np.int64), b.normal.view(np.int64))
        T.check_planes(pls, f["planes"])
        assert info["n_own"] == info["n_local"] == info["n_grow"] == n and info["halo_retries"] == 0
        assert info["planes_total"] == len(planes)


def _same(a, b):
    for (la, ia, pa), (lb, ib, pb) in zip(a, b):
        assert np.array_equal(la, lb)
        for key in SAME_ON_EVERY_RANK + ("n_own", "n_local", "n_grow"):
            assert ia[key] == ib[key], key
        assert [q.id for q in pa] == [q.id for q in pb]
        for x, y in zip(pa, pb):
            assert np.array_equal(x.pointIdx, y.pointIdx) and np.array_equal(x.center, y.center)
            assert np.array_equal(x.normal.view(np.int64), y.normal.view(np.int64))


def test_reuse_of_contexts_and_communicator(oracle, ctxs):
    """A (small, two components on three ranks), B (the largest cloud), C (one component: two ranks grow nothing right
    after a call that left planes on them), A again -- on the same three contexts and ONE communicator."""
    import dataclasses
    a = dataclasses.replace(S.BY_NAME["far_boxes_w2"], world=3, rule="interleaved")
    b = dataclasses.replace(S.BY_NAME["boxes6_random_w4"], world=3)
    c = S.BY_NAME["disc_retry1_w3"]
    assert len(S.cloud(b)) == max(len(S.cloud(sc)) for sc in S.SCENARIOS) and len(S.cloud(a)) < len(S.cloud(b)) // 3
    comm = T.Comm(3)
    try:
        runs = []
        for sc in (a, b, c, a):
            f, _, res = _run(ctxs, comm, sc, oracle)
            _check(res, f, sc)
            runs.append(res)
    finally:
        comm.close()
    idle = [r for r in range(3) if runs[2][r][1]["n_grow"] == 0]
    assert len(idle) == 2 and all(runs[2][r][2] == [] for r in idle)  # C's idle ranks fetch the empty set ...
    assert all(len(runs[1][r][2]) > 0 for r in idle)  # ... although B had left planes on them
    _same(runs[0], runs[3])
    assert any(x[1]["n_grow"] == 0 for x in runs[0])  # (A itself has an idle rank: two components on three ranks)


def _raised(res, status):
    from buildingsegment_amd import api
    for r, x in enumerate(res):
        assert isinstance(x, api.BsError), f"rank {r} returned {type(x)}"
        assert x.status == status, f"rank {r}: {x}"


def test_errors_reach_every_rank_and_the_next_call_succeeds(oracle, ctxs):
    good = S.BY_NAME["boxes3_k32_w3"]
    world = good.world
    comm = T.Comm(world)
    try:
        # (a) the shares miss one point: rank 0 passes its share without its last point, n_total stays
        f = S.facts(oracle, good)
        n = len(f["xyz"])
        parts = S.shares(good.rule, n, world)
        parts[0] = parts[0][:-1]
        assert len(np.concatenate(parts)) == n - 1 and np.concatenate(parts).max() < n
        t0 = time.monotonic()
        res = T.run_ranks(ctxs[:world], comm, f["xyz"], parts, _params(good), good.halo, n_total=n)
        _raised(res, BS_ERR_INVALID)
        assert time.monotonic() - t0 < T.COMM_TIMEOUT_S / 2  # agreed on, nobody waited for the deadline
        assert all("cover the cloud exactly once" in str(x) for x in res)
        # (c) the same contexts and communicator still work
        f, _, res = _run(ctxs, comm, good, oracle)
        _check(res, f, good)
        # (b) no halo within six doublings certifies the coarse lattice
        bad = S.BY_NAME["coarse_lattice_uncertified_w2"]
        import dataclasses
        bad = dataclasses.replace(bad, world=world)
        fb = S.facts(oracle, bad)
        assert fb["retries"] is None
        t0 = time.monotonic()
        res = T.run_ranks(ctxs[:world], comm, fb["xyz"], S.shares(bad.rule, len(fb["xyz"]), world), _params(bad), bad.halo)
        _raised(res, BS_ERR_UNCERTIFIED)
        assert time.monotonic() - t0 < T.COMM_TIMEOUT_S / 2
        f, _, res = _run(ctxs, comm, good, oracle)
        _check(res, f, good)
        # a share that only its own rank can see is wrong (no global indices at world 3): that rank reports it, the
        # others learn of it in the first all-reduce -- at once, and the communicator stays usable
        parts = S.shares(good.rule, n, world)
        res = _run_without_gidx_on_rank(ctxs[:world], comm, f["xyz"], parts, _params(good), good.halo, rank=1)
        from buildingsegment_amd import api
        assert all(isinstance(x, api.BsError) for x in res), res
        assert [x.status for x in res] == [BS_ERR_INTERNAL, BS_ERR_INVALID, BS_ERR_INTERNAL]
        assert "d_gidx is required" in str(res[1]) and "another rank passed bad arguments" in str(res[0])
        f, _, res = _run(ctxs, comm, good, oracle)
        _check(res, f, good)
    finally:
        comm.close()


def _run_without_gidx_on_rank(ctxs, comm, xyz, parts, params, halo, rank):
    import torch
    dev = torch.device("cuda", 0)
    n = len(xyz)
    res = [None] * comm.world
    t0 = time.monotonic()

    def run(r):
        try:
            d_xyz = torch.from_numpy(np.ascontiguousarray(xyz[parts[r]])).to(dev)
            d_g = torch.from_numpy(parts[r].copy()).to(dev)
            d_lab = torch.empty(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctxs[r].segment_sharded(comm.ops[r], d_xyz.data_ptr(), 0 if r == rank else d_g.data_ptr(), len(parts[r]), n,
                                    d_lab.data_ptr(), params, halo=halo)
            res[r] = "returned"
        except Exception as e:  # noqa: BLE001
            res[r] = e

    ts = [threading.Thread(target=run, args=(r,)) for r in range(comm.world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=T.JOIN_S)
    assert not any(t.is_alive() for t in ts)
    assert time.monotonic() - t0 < T.COMM_TIMEOUT_S / 2
    return res


def test_barrier_deadline_of_the_in_process_communicator(gpu_ctx, monkeypatch):
    """Only rank 0 of a world-2 communicator enters an all-reduce (called through the ops table on an 8-byte device
    buffer).  With BS_COMM_LOCAL_TIMEOUT_S=2 the call returns non-zero after about two seconds, and every later
    collective on either rank returns non-zero at once: the communicator is broken for good.  The GPU is idle
    throughout -- what times out is the wait on a host condition variable, no kernel and no copy is in flight."""
    import torch
    monkeypatch.setenv("BS_COMM_LOCAL_TIMEOUT_S", "2")
    comm = T.Comm(2)
    monkeypatch.setenv("BS_COMM_LOCAL_TIMEOUT_S", "600")  # read at creation: a later value changes nothing
    try:
        buf = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        AR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p)
        AG = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
        BS_I64, BS_SUM = 1, 2
        out = []

        def alone():
            t0 = time.monotonic()
            rc = AR(comm.ops[0].all_reduce)(comm.ops[0].handle, buf.data_ptr(), 1, BS_I64, BS_SUM, None)
            out.append((rc, time.monotonic() - t0))

        t = threading.Thread(target=alone)
        t.start()
        t.join(timeout=30)
        assert not t.is_alive()
        rc, dt = out[0]
        assert rc != 0 and 1.5 < dt < 10.0, (rc, dt)
        for r in (1, 0):  # later calls: non-zero, without waiting
            t0 = time.monotonic()
            assert AR(comm.ops[r].all_reduce)(comm.ops[r].handle, buf.data_ptr(), 1, BS_I64, BS_SUM, None) != 0
            assert AG(comm.ops[r].all_gather)(comm.ops[r].handle, buf.data_ptr(), buf.data_ptr() + 8, 0, None) != 0
            assert time.monotonic() - t0 < 1.0
    finally:
        comm.close()
