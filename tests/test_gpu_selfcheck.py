"""The grower's built-in self-checks (BS_VERIFY=1) stay silent on real runs.

BS_VERIFY makes bs_grow_spec.hip re-derive, with independent kernels, two things the fast path
maintains incrementally: the orphan-maker owner structure (is it a fixed point of its equations?)
and the per-point records (do they equal a full refresh after every round?).  A mismatch prints a
`[bs] VERIFY:` line on stderr.  The check runs in a child process because the switch is read from
the environment."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, glob, os
import numpy as np
sys.path.insert(0, sys.argv[1])
from buildingsegment_amd import api, synth
ctx = api.Context(0)
rounds = 0
for name, xyz, k in (("plane_cube", synth.plane_cube(), 15), ("facade", synth.facade(550, seed=3), 16),
                     ("urban", synth.urban(600_000, seed=5), 16)):
    p = api.default_params(k=k)
    neigh, normals, plane_idx, planes = ctx.segment(np.ascontiguousarray(xyz), p)
    rounds += ctx.timings()["rg_rounds"]
    assert int((plane_idx >= 0).sum()) > 0, name
print("rounds", rounds)
"""


def test_incremental_structures_match_their_definitions():
    env = dict(os.environ, BS_VERIFY="1")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rounds" in out.stdout
    assert "VERIFY:" not in out.stderr, out.stderr


ORDER_CHILD = r"""
import sys, hashlib
import numpy as np
sys.path.insert(0, sys.argv[1])
from buildingsegment_amd import api, synth
ctx = api.Context(0)
ctx.set_audit(True)
xyz = np.ascontiguousarray(synth.urban(4_000_000, seed=11))
neigh, normals, plane_idx, planes = ctx.segment(xyz, api.default_params(k=16))
tm = ctx.timings()
h = hashlib.sha256()
h.update(plane_idx.tobytes())
for p in planes:
    h.update(p.pointIdx.tobytes()); h.update(p.normal.tobytes()); h.update(np.asarray(p.center).tobytes())
print("RESULT", h.hexdigest(), len(planes), tm["n_seed_attempts"], tm["audit_attempts"], tm["audit_mismatches"], tm["rg_rounds"])
"""


def _order_child(extra):
    """Runs ORDER_CHILD with `extra` in the environment; returns its digest and stderr (the audit must agree)."""
    out = subprocess.run([sys.executable, "-c", ORDER_CHILD, ROOT], capture_output=True, text=True,
                         env=dict(os.environ, **extra), timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][0].split()
    digest, n_planes, attempts, audited, mism = line[1], int(line[2]), int(line[3]), int(line[4]), int(line[5])
    assert mism == 0 and audited == attempts >= n_planes > 0, line
    return digest, out.stderr


def test_big_round_scheduling_switches_do_not_change_the_result():
    """Rounds with >= 4096 attempts use a dispatch order (tile leaders first) and send only the finished attempts
    to the host.  Both are pure scheduling: with the dispatch order switched off (BS_NO_DISPATCH_ORDER) and with
    the debug path that moves every attempt (BS_DEBUG) the labels, lists, normals and centres are the same bits,
    and the audit replay agrees each time.  4 M-point urban scene (about 10 k attempts in the first round)."""
    results = []
    for extra in ({}, {"BS_NO_DISPATCH_ORDER": "1"}, {"BS_DEBUG": "1"}):
        digest, err = _order_child(extra)
        if extra.get("BS_DEBUG"):
            assert "ncand_all=" in err
            big = [int(l.split("ncand_all=")[1].split()[0]) for l in err.splitlines() if "ncand_all=" in l]
            assert max(big) >= 4096, "the scene is too small to exercise the big-round paths"
        results.append(digest)
    assert results[0] == results[1] == results[2]


def test_first_step_engine_fallback_gives_the_same_bits():
    """BS_GROW_V2=0 puts every k <= 16 round on the first step engine (grow_spec_kernel<16>), the fallback of the
    default grow_spec2_kernel<16>; the audit replay follows the switch.  On the scene above (a first round of about
    10 k attempts) the labels, lists, normals and centres are the same bits with either engine."""
    assert _order_child({})[0] == _order_child({"BS_GROW_V2": "0"})[0]
