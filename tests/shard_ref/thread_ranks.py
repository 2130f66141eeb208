"""Thread-ranks on one GPU for the tests of bs_segment_sharded: every rank is a thread of the test process with its own
context, the ranks talk through bs_comm_local_create.  Shared by tests/test_gpu_sharded_capi.py and
tests/test_gpu_sharded_scenarios.py."""
import ctypes as C
import threading
import time

import numpy as np

COMM_TIMEOUT_S = 60  # BS_COMM_LOCAL_TIMEOUT_S of the scenario tests: a rank left alone gives up after a minute ...
JOIN_S = 90          # ... and the test waits longer than that for its threads


def expected(oracle, xyz, k):
    ng, nr = oracle.knn_normals(xyz, k=k)
    pi, pl = oracle.region_grow(xyz, nr, ng)
    return pi, pl


def check_planes(all_planes, pl):
    """The ranks' planes together are the oracle's, each exactly once: id, pointIdx, centre, the normal's 64-bit pattern."""
    all_planes = sorted(all_planes, key=lambda q: q.id)
    assert [q.id for q in all_planes] == pl["id"].tolist()
    off = pl["offset"]
    for i, q in enumerate(all_planes):
        assert np.array_equal(q.pointIdx, pl["point_idx"][off[i]:off[i + 1]])
        assert np.array_equal(q.center, pl["center"][i])
        assert np.array_equal(q.normal.view(np.int64), pl["normal"][i].view(np.int64))


class Comm:
    """One in-process communicator of `world` ranks."""

    def __init__(self, world):
        from buildingsegment_amd import _lib
        self.L = _lib.load()
        self.world = world
        self.ops = (_lib.CommOps * world)()
        assert self.L.bs_comm_local_create(world, self.ops) == 0

    def close(self):
        for r in range(self.world):
            self.L.bs_comm_local_destroy(C.byref(self.ops[r]))


def run_ranks(ctxs, comm, xyz, parts, params, halo, n_total=None, join_s=JOIN_S):
    """Rank r = a thread that passes xyz[parts[r]] with the global indices parts[r] (an empty share: null pointers) to
    bs_segment_sharded on ctxs[r].  -> per rank (labels [n_total], info, planes of this rank) or the exception raised.
    No thread is left behind: one that is still running after join_s seconds fails the test."""
    import torch
    world = comm.world
    n = len(xyz) if n_total is None else n_total
    dev = torch.device("cuda", 0)
    res = [None] * world

    def run(r):
        try:
            idx = np.ascontiguousarray(parts[r], dtype=np.int32)
            m = len(idx)
            d_xyz = torch.from_numpy(np.ascontiguousarray(xyz[idx])).to(dev) if m else None
            d_g = torch.from_numpy(idx.copy()).to(dev) if m else None
            d_lab = torch.empty(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            info = ctxs[r].segment_sharded(comm.ops[r], d_xyz.data_ptr() if m else 0, d_g.data_ptr() if m else 0, m, n,
                                           d_lab.data_ptr(), params, halo=halo)
            res[r] = (d_lab.cpu().numpy(), info, ctxs[r].sharded_planes_fetch())
        except Exception as e:  # noqa: BLE001
            res[r] = e

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    end = time.monotonic() + join_s
    for t in ts:
        t.join(timeout=max(0.0, end - time.monotonic()))
    assert not any(t.is_alive() for t in ts), "a thread-rank is still inside bs_segment_sharded"
    return res
