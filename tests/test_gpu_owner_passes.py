"""The owner passes of the speculative grower under every schedule.

pull_list_kernel (bs_grow_spec.hip) re-evaluates the dirty points of the orphan-maker owner structure from a worklist
of dirty 256-point groups that the workgroups of a pass share evenly (the mechanism is described at wl_flush there),
reading a reverse list 16 edges per trip; cand_flag_kernel reads all owners of a row in one trip; the decide passes
of the first fixed point are unchanged kernels launched in groups with one host round trip per group.  The schedule
cannot change the result (the owner equations have one fixed point), so every case here is compared with the CPU
oracle bit for bit -- labels, every plane's list, centre and normal, and the owner of every point -- with the audit
replay on (0 mismatches, as many attempts as the rounds finalised), and is followed by one plain call on the same
context: nothing of a forced geometry may stay behind.

Switches (read per call): BS_OWNER_WORKLIST=0 = the dirty groups found by their flags, a fixed range per workgroup
(pull_pass_kernel); BS_OWNER_GRID = workgroups per pass (1: one workgroup walks every list: more listed groups than
workgroups on any cloud above 512 points); BS_OWNER_GROUP = passes per host round trip (2: every settle crosses the
boundary between two groups of launches several times, the worklist has to carry over).

Inputs are the smallest at which each mechanism can go wrong:
 - the clouds of tests/test_gpu_grow_limits.py (100 k - 400 k points: hundreds of groups, big first rounds; fuzz_7_106:
   hundreds of rounds of insert / drop settles);
 - a hub cloud: two jittered sheets whose k = 16 rows are rewritten so that one point (three in the second variant) is
   named by ~90 % (~30 %) of all rows -- reverse lists of thousands of entries, far beyond one 16-edge trip, next to
   lists of 17-24 (trip + remainder) and the ordinary ones below 16;
 - 63, 255, 256 and 257 points of a sheet: less than a wave, a partial group, exactly one group, one group and a point.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from buildingsegment_amd import api

from test_gpu_grow_limits import _audit_ok, _equal_oracle, _input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCHEDULES = {
    "default": {},
    "flagscan": {"BS_OWNER_WORKLIST": "0"},
    "grid1": {"BS_OWNER_GRID": "1"},
    "grid2": {"BS_OWNER_GRID": "2"},
    "group2": {"BS_OWNER_GROUP": "2"},
    "grid1_group2": {"BS_OWNER_GRID": "1", "BS_OWNER_GROUP": "2"},
}
SWITCHES = ("BS_OWNER_WORKLIST", "BS_OWNER_GRID", "BS_OWNER_GROUP")


def _schedule(monkeypatch, name):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for k, v in SCHEDULES[name].items():
        monkeypatch.setenv(k, v)


def _owners(ctx, n):
    import torch
    d_own = torch.empty(n, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.owner_fetch_dev(d_own.data_ptr())
    ctx.sync()
    return d_own.cpu().numpy()


_OWNER = {}


def _case(O, key, xyz, normals, neigh, kw):
    """Oracle result of an input, computed once: (labels, planes), owners."""
    if key not in _OWNER:
        full = {"th_thickness": 300, "th_point_count": 400, "cos_th": 0.88, **kw}
        pi, pl, ow = O.region_grow(xyz, normals, neigh, want_owner=True, **full)
        _OWNER[key] = ((pi, pl), ow)
    return _OWNER[key]


def _orphans(want, owner):
    """points left labelled by an attempt that committed no plane"""
    seeds = want[1]["point_idx"][want[1]["offset"][:-1]]
    return int(((owner >= 0) & ~np.isin(owner, seeds)).sum())


def _check(ctx, monkeypatch, schedule, xyz, normals, neigh, kw, want, owner):
    p = api.default_params(k=neigh.shape[1], rg_mode=2, **kw)
    _schedule(monkeypatch, schedule)
    ctx.set_audit(True)
    try:
        pi, planes = ctx.region_grow(xyz, normals, neigh, p)
        _audit_ok(ctx)
        _equal_oracle(pi, planes, want)
        assert np.array_equal(_owners(ctx, len(xyz)), owner)
    finally:
        ctx.set_audit(False)
    _schedule(monkeypatch, "default")  # one plain call: the same result, nothing left behind
    pi, planes = ctx.region_grow(xyz, normals, neigh, p)
    _equal_oracle(pi, planes, want)
    assert np.array_equal(_owners(ctx, len(xyz)), owner)


# ---- 1. schedules agree ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", tuple(SCHEDULES))
@pytest.mark.parametrize("name", ("plane_cube_k15", "facade400_k16", "urban400k_k16", "fuzz_7_106"))
def test_schedules_agree(gpu_ctx, oracle, monkeypatch, name, schedule):
    xyz, normals, neigh, kw, _ = _input(oracle, name)
    want, owner = _case(oracle, name, xyz, normals, neigh, kw)
    assert len(xyz) > 512
    _check(gpu_ctx, monkeypatch, schedule, xyz, normals, neigh, kw, want, owner)


# ---- 2. long reverse lists -------------------------------------------------------------------------------------

def _sheet(rng, nx, ny, z0, znoise):
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    m = nx * ny
    return np.stack([gx.ravel() * 50 + rng.integers(-10, 11, m), gy.ravel() * 50 + rng.integers(-10, 11, m),
                     z0 + rng.integers(-znoise, znoise + 1, m)], axis=1)


_HUB = {}


def _hub_cloud(O, hubs):
    """Two jittered sheets (37 x 41 and 30 x 30 points, 50 mm spacing, the second at z = 3000) in one shuffled cloud
    with k = 16 rows; slot 15 of ~90 % of the rows names one hub, and with three hubs slots 14 and 13 of ~30 % of the
    rows name two more.  A row that is a hub or already holds it is left alone: no row holds an index twice."""
    if hubs not in _HUB:
        rng = np.random.default_rng(11)
        xyz = np.concatenate([_sheet(rng, 37, 41, 0, 5), _sheet(rng, 30, 30, 3000, 5)])
        xyz = np.ascontiguousarray(xyz[rng.permutation(len(xyz))], dtype=np.int32)
        n = len(xyz)
        neigh, normals = O.knn_normals(xyz, k=16)
        neigh = neigh.copy()
        plan = [(15, n // 2, 0.9)] + ([(14, n // 3, 0.3), (13, n // 5, 0.3)] if hubs == 3 else [])
        for slot, hub, share in plan:
            pick = rng.random(n) < share
            pick &= ~(neigh == hub).any(axis=1) & (np.arange(n) != hub)
            neigh[pick, slot] = hub
        srt = np.sort(neigh, axis=1)
        assert not (srt[:, 1:] == srt[:, :-1]).any()
        _HUB[hubs] = (xyz, np.ascontiguousarray(normals), np.ascontiguousarray(neigh))
    return _HUB[hubs]


@pytest.mark.parametrize("schedule", ("default", "grid1"))
@pytest.mark.parametrize("th_point_count", (0, 40))
@pytest.mark.parametrize("hubs", (1, 3))
def test_long_reverse_lists(gpu_ctx, oracle, monkeypatch, hubs, th_point_count, schedule):
    xyz, normals, neigh = _hub_cloud(oracle, hubs)
    kw = dict(th_point_count=th_point_count)
    want, owner = _case(oracle, ("hub", hubs, th_point_count), xyz, normals, neigh, kw)
    # the input is what it is for (in-degrees over the rows: the static masks can only shorten a reverse list, and
    # the equality with the oracle's owners below is what the long lists are checked by)
    indeg = np.bincount(neigh[:, 1:].ravel(), minlength=len(xyz))
    print(f"HUB hubs={hubs} cnt={th_point_count} n={len(xyz)} planes={len(want[1]['id'])} attempts={want[1]['n_seed_attempts']} "
          f"orphans={_orphans(want, owner)} longest={indeg.max()} above16={(indeg > 16).sum()}")
    assert len(want[1]["id"]) >= 1 and want[1]["n_seed_attempts"] >= 100
    assert _orphans(want, owner) >= 500 and indeg.max() >= 1024 and (indeg > 16).sum() > 16
    _check(gpu_ctx, monkeypatch, schedule, xyz, normals, neigh, kw, want, owner)


# ---- 3. group edges --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", (63, 255, 256, 257))
def test_group_edges(gpu_ctx, oracle, monkeypatch, m):
    rng = np.random.default_rng(3)
    sheet = _sheet(rng, 17, 17, 0, 20)
    xyz = np.ascontiguousarray(sheet[rng.permutation(len(sheet))][:m], dtype=np.int32)
    neigh, normals = oracle.knn_normals(xyz, k=16)
    kw = dict(th_point_count=20)
    want, owner = _case(oracle, ("edge", m), xyz, normals, neigh, kw)
    print(f"EDGE m={m} planes={len(want[1]['id'])} attempts={want[1]['n_seed_attempts']} orphans={_orphans(want, owner)}")
    if m >= 255:
        assert len(want[1]["id"]) >= 1 and want[1]["n_seed_attempts"] >= 5 and _orphans(want, owner) >= 10
    for schedule in ("default", "grid1_group2"):
        _check(gpu_ctx, monkeypatch, schedule, xyz, normals, np.ascontiguousarray(neigh), kw, want, owner)


# ---- 4. the definitions hold -----------------------------------------------------------------------------------

VERIFY_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from buildingsegment_amd import api, synth
ctx = api.Context(0)
rounds = 0
for name, xyz, k in (("plane_cube", synth.plane_cube(), 15), ("facade", synth.facade(400, seed=9), 16)):
    neigh, normals, plane_idx, planes = ctx.segment(np.ascontiguousarray(xyz), api.default_params(k=k))
    rounds += ctx.timings()["rg_rounds"]
    assert int((plane_idx >= 0).sum()) > 0, name
g = np.load(sys.argv[2])
for cnt in (0, 40):
    ctx.region_grow(g["xyz"], g["normals"], g["neigh"], api.default_params(k=16, rg_mode=2, th_point_count=cnt))
    rounds += ctx.timings()["rg_rounds"]
print("rounds", rounds)
"""


@pytest.mark.parametrize("schedule", ("default", "grid1_group2"))
def test_definitions_hold(oracle, tmp_path, schedule):
    """BS_VERIFY=1 (verify_fixpoint_kernel after every settle, verify_records_kernel before every round: the
    independent definitions of what the passes maintain) stays silent; in a child process, the switch is read from
    the environment.  The child prints the sum of the round counts: an early exit cannot pass silently."""
    xyz, normals, neigh = _hub_cloud(oracle, 3)
    f = str(tmp_path / "hub.npz")
    np.savez(f, xyz=xyz, normals=normals, neigh=neigh)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(SCHEDULES[schedule], BS_VERIFY="1")
    out = subprocess.run([sys.executable, "-c", VERIFY_CHILD, ROOT, f], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("rounds")]
    assert line and int(line[0].split()[1]) >= 4, out.stdout
    assert "VERIFY:" not in out.stderr, out.stderr[-3000:]
