"""The speculative grower when a resource runs out: every capacity limit of bs_grow_spec.hip crossed at test size.

The grower's recovery paths -- a round that grows only the lowest candidates, a round pool that is exhausted
(ST_NOMEM: full record refresh, attempts per round cut to an eighth, BS_ERR_NOMEM at one attempt), finished planes
that find no pending slot or no room in the pending store, a stolen plane that waits for the next round -- are sized
so that they only fire on clouds of 10^8 points.  bs_selftest_grow_limits lowers the limits; bs_get_grow_counters
tells which of them the host loop saw reached.  Every test here lowers one limit, REQUIRES the matching counter to be
positive (a limit that was not reached is a failure, not a pass), compares labels, plane count, every plane's list,
centre and normal with the CPU oracle bit for bit, runs the audit replay (0 mismatches, as many attempts as the rounds
finalised), and then repeats the call without the hook on the same context: nothing may be left behind.

Engines (chosen by k in launch_region_grow_spec): "v2" = grow_spec2_kernel<16>, the default at k <= 16; "v1" =
grow_spec_kernel<16> (BS_GROW_V2=0, read per call); "k32" = grow_spec_kernel<32> at 16 < k <= 32.

Not counted: the in-launch re-growths of one attempt (PlaneOut has no free word at the end of an attempt: pad is the
host's command for plane_apply_kernel, pad4 the failed test of validate2, pad5 the hardware id), so the re-growth
policies are checked by their results and by attempts_stolen alone.

LIFO window.  The oracle keeps the pending Broad() calls of the reference's recursion in an explicit LIFO
(oracle/bs_oracle.c, region_grow_core, `stack`): a call pushes the points it accepted in reverse selection order and
the next call is the popped top.  Both device engines do the same with `sp`: the expanded call's children go to
sp + (cnt - 1 - rank) (first child on top), then sp += cnt; the pops are sp -= last + 1, where the multi-pop consumes
the run of `last` pending calls that accept nothing together with the one that is expanded -- calls the oracle pops
one by one, pushing nothing in between.  So after every expanded call the device's sp equals the oracle's stack.n
after the same call's pushes, and the peak of stack.n is the peak of sp.  The device keeps entries
[lds_lo, sp) in LDS (LDS_STACK = 256) and brings LDS_REFILL = 128 back when a pop reaches below lds_lo; the first
engine moves lds_lo exactly like the oracle-side model (lds_lo = sp - 256 after the pushes), the default engine writes
the older half of the window out instead, so the model's event counts are not the device's -- they state that the
input drives the stack far above the window and back below it many times.

Wall time on the MI355X: 72 s for the whole file, 54 tests (21 s of it the 40 fuzz cases with random limits, 18 s the
clouds of ~1 000 and ~2 100 rounds under four policies and in big rounds); tests/test_gpu_parity.py takes 43 s in the
same run of the suite on the same machine.  Nothing had to be reduced.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from buildingsegment_amd import api, synth
from buildingsegment_amd._lib import BsError

from test_gpu_batch import _oracle as _tile_oracle, _same, _tiny_tiles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

ENGINES = ("v2", "v1", "k32")


def _engine(monkeypatch, engine):
    if engine == "v1":
        monkeypatch.setenv("BS_GROW_V2", "0")
    else:
        monkeypatch.delenv("BS_GROW_V2", raising=False)


# ---- inputs: (xyz, normals, neigh, grow parameters, oracle result), built once per session ----------------------

_CACHE = {}


def _fuzz_7_106(strip=False):
    g = np.load(os.path.join(ROOT, "tests", "data", "fuzz_fail_7_106.npz"))
    kw = dict(th_thickness=int(g["th"]), th_point_count=int(g["cnt"]), cos_th=float(g["cos"]))
    if not strip:
        return g["xyz"], g["normals"], g["neigh"], kw
    # the strip x < 600 mm of the 4 m sheet (a prefix of the shuffled cloud is too sparse to grow anything): 3 746
    # points with k-lists of their own, 2 801 attempts, 2 committed planes (429 and 441 entries) in the oracle
    m = g["xyz"][:, 0] < 600
    return g["xyz"][m], g["normals"][m], None, kw


def _fuzz_2718_16():
    """Fuzz case 2718/16 the way `fuzz_parity.py --seed 2718 --only 16` draws it (29 077 points, k = 21, thickness 2000,
    th_point_count 0); in the normals' place: the case's normal noise (None: the normals stay as computed)."""
    import fuzz_parity
    xyz, kw, noise = fuzz_parity.replay_case(2718, 16)
    return xyz, noise, None, {key: kw[key] for key in ("th_thickness", "th_point_count", "cos_th")}, kw["k"]


def _fuzz_7_106_twice():
    """Two copies of fuzz_fail_7_106, 1 km apart, as one cloud of 49 850 points (the second copy's k-lists shifted by
    n): one copy alone has more than 3 179 candidates in its first rounds (rounds_capped > 0 at that cap), two have
    more than 4096 -- rounds big enough for the dispatch order and the compacted copy-back, with an oracle."""
    xyz, normals, neigh, kw = _fuzz_7_106()
    far = xyz + np.array([1_000_000, 0, 0], dtype=xyz.dtype)
    return (np.concatenate([xyz, far]), np.concatenate([normals, normals]), np.concatenate([neigh, neigh + len(xyz)]), kw, 4)


_MAKERS = {
    "fuzz_7_106": lambda: _fuzz_7_106() + (4,),
    "fuzz_7_106_twice": _fuzz_7_106_twice,
    "fuzz_7_106_strip": lambda: _fuzz_7_106(True) + (4,),
    "fuzz_2718_16": _fuzz_2718_16,
    "plane_cube_k15": lambda: (synth.plane_cube(), None, None, {}, 15),
    "plane_cube_k32": lambda: (synth.plane_cube(), None, None, {}, 32),
    "facade400_k16": lambda: (synth.facade(400, seed=9), None, None, {}, 16),
    "urban400k_k16": lambda: (synth.urban(400_000, seed=9), None, None, dict(th_point_count=0), 16),
    "boxes_k32": lambda: (synth.boxes(), None, None, {}, 32),
}


def _input(O, name):
    """xyz, normals, neigh, kw, (oracle labels, oracle planes, LIFO model [n_planes, 4])"""
    if name not in _CACHE:
        xyz, normals, neigh, kw, k = _MAKERS[name]()
        xyz = np.ascontiguousarray(xyz, dtype=np.int32)
        if neigh is None:
            neigh, own = O.knn_normals(xyz, k=k)
            if name == "fuzz_2718_16":
                import fuzz_parity
                normals = fuzz_parity.perturb(own, normals)  # (normals holds the case's noise, or None)
            elif normals is None:
                normals = own
        normals = np.ascontiguousarray(normals, dtype=np.float64)
        opi, opl, lifo = O.region_grow(xyz, normals, neigh, want_lifo=True, **{"th_thickness": 300, "th_point_count": 400,
                                                                              "cos_th": 0.88, **kw})
        _CACHE[name] = (xyz, normals, np.ascontiguousarray(neigh), kw, (opi, opl, lifo))
    return _CACHE[name]


INPUTS = {"v2": ("plane_cube_k15", "facade400_k16", "urban400k_k16"),
          "v1": ("plane_cube_k15", "facade400_k16", "urban400k_k16"),
          "k32": ("plane_cube_k32", "boxes_k32")}


def _equal_oracle(pi, planes, want):
    opi, opl = want[0], want[1]
    assert np.array_equal(pi, opi), f"{(pi != opi).sum()} labels differ"
    assert len(planes) == len(opl["id"])
    for i, pl in enumerate(planes):
        assert pl.id == opl["id"][i]
        assert np.array_equal(pl.pointIdx, opl["point_idx"][opl["offset"][i]:opl["offset"][i + 1]])
        assert np.array_equal(pl.center, opl["center"][i])
        assert np.array_equal(pl.normal, opl["normal"][i])


def _audit_ok(ctx):
    tm = ctx.timings()
    assert tm["audit_mismatches"] == 0 and tm["audit_attempts"] == tm["n_seed_attempts"], tm
    return tm


SHOW = ("rounds", "rounds_capped", "rounds_big", "attempts_nomem", "waves_cut", "max_waves_end", "attempts_stolen",
        "dropped_pend_count", "dropped_pend_store", "dropped_other", "full_refreshes")


def _show(what, lim, gc):
    print(f"LIMITS {what} | {' '.join(f'{k}={v}' for k, v in lim.items())} | " + " ".join(f"{k}={gc[k]}" for k in SHOW))


def _grow(ctx, O, name, lim, what, unhooked_after=True):
    """One audited region grow of input `name` with the limits `lim`; equal to the oracle; returns the counters."""
    xyz, normals, neigh, kw, want = _input(O, name)
    p = api.default_params(k=neigh.shape[1], rg_mode=2, **kw)
    ctx.set_audit(True)
    try:
        ctx.selftest_grow_limits(**lim)
        pi, planes = ctx.region_grow(xyz, normals, neigh, p)
        gc = ctx.grow_counters()
        _show(f"{what} {name}", lim, gc)
        gc["n_seed_attempts"] = _audit_ok(ctx)["n_seed_attempts"]
        _equal_oracle(pi, planes, want)
        assert gc["rounds"] == ctx.timings()["rg_rounds"]
    finally:
        ctx.selftest_grow_limits()
        ctx.set_audit(False)
    if unhooked_after and lim:
        _unhooked(ctx, O, name)
    return gc


def _unhooked(ctx, O, name):
    """The context carries nothing over: without the hook the same call is the oracle's result, at default limits."""
    xyz, normals, neigh, kw, want = _input(O, name)
    pi, planes = ctx.region_grow(xyz, normals, neigh, api.default_params(k=neigh.shape[1], rg_mode=2, **kw))
    _equal_oracle(pi, planes, want)
    gc = ctx.grow_counters()
    # (dropped_pend_store is not asserted: fuzz_fail_7_106 fills the DEFAULT store, 6 n + 65 536 entries, in every run)
    assert gc["attempts_nomem"] == 0 and gc["waves_cut"] == 0 and gc["dropped_pend_count"] == 0, gc
    return gc


# ---- 1. capped rounds ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_waves", (7, 64, 4096))
@pytest.mark.parametrize("engine", ("v2", "v1"))
def test_capped_rounds_many_attempts(gpu_ctx, oracle, monkeypatch, engine, max_waves):
    """fuzz_fail_7_106: 24 925 points, k = 4, ~18 000 plane attempts, 10 committed planes.  Only the lowest max_waves
    candidates of a round are grown.  (The per-attempt arrays hold n / 8 + 64 = 3 179 attempts, so 4096 is clamped
    to that: still far below the candidates of the first rounds.)"""
    _engine(monkeypatch, engine)
    gc = _grow(gpu_ctx, oracle, "fuzz_7_106", dict(max_waves=max_waves), f"capped[{engine}]")
    assert gc["rounds_capped"] > 0
    assert gc["max_waves_end"] == min(max_waves, 24925 // 8 + 64)


@pytest.mark.parametrize("engine", ("v2", "v1"))
def test_one_attempt_per_round(gpu_ctx, oracle, monkeypatch, engine):
    """max_waves = 1: the grower degenerates to the reference's sequential order, one attempt per round, on a strip
    of fuzz_fail_7_106 (3 746 points, 2 committed planes; the whole cloud would take ~19 000 rounds)."""
    _engine(monkeypatch, engine)
    _, _, _, _, want = _input(oracle, "fuzz_7_106_strip")
    gc = _grow(gpu_ctx, oracle, "fuzz_7_106_strip", dict(max_waves=1), f"capped[{engine}]")
    assert gc["rounds_capped"] > 0 and gc["max_waves_end"] == 1
    assert len(want[1]["id"]) == 2 and len(_input(oracle, "fuzz_7_106_strip")[0]) == 3746
    assert want[1]["n_seed_attempts"] == 2801  # (the oracle also counts seeds that can never pass depth 0)
    assert gc["rounds"] >= gc["n_seed_attempts"] > 2000  # every attempt the rounds finalised had a round of its own


@pytest.mark.parametrize("max_waves", (1, 7, 64))
def test_capped_rounds_k32_engine(gpu_ctx, oracle, max_waves):
    """The same on grow_spec_kernel<32>: boxes() at k = 32 (6 463 attempts, 6 committed planes of 2 246-2 740)."""
    gc = _grow(gpu_ctx, oracle, "boxes_k32", dict(max_waves=max_waves), "capped[k32]")
    assert gc["rounds_capped"] > 0 and gc["max_waves_end"] == max_waves


def test_audit_fits_the_pool_when_the_environment_caps_the_rounds(gpu_ctx, oracle, monkeypatch):
    """Regression (found by the tests above): the round pool was sized for max_waves attempts while the audit replays
    n / 8 + 64 per batch, so with BS_MAX_WAVES (or the hook) below that the replays ended ST_NOMEM and a CORRECT grow
    failed with BS_ERR_INTERNAL "audit: a batch of rolled-back attempts made no progress"."""
    monkeypatch.setenv("BS_MAX_WAVES", "1")
    gc = _grow(gpu_ctx, oracle, "fuzz_7_106_strip", {}, "env BS_MAX_WAVES=1", unhooked_after=False)
    assert gc["rounds_capped"] > 0 and gc["max_waves_end"] == 1
    monkeypatch.setenv("BS_MAX_WAVES", "64")
    gc = _grow(gpu_ctx, oracle, "fuzz_7_106", dict(max_waves=7), "env BS_MAX_WAVES=64, hook 7", unhooked_after=False)
    assert gc["max_waves_end"] == 7  # (the hook wins over the environment)


@pytest.mark.parametrize("engine", ("v2", "v1"))
def test_big_rounds_against_the_oracle(gpu_ctx, oracle, monkeypatch, engine):
    """Rounds of 4096 attempts or more (dispatch order by tile leaders, only finished and exhausted attempts copied
    back) compared with the ORACLE, not with another run: two copies of fuzz_fail_7_106 in one cloud, at the default
    limits, and with the rounds capped at exactly 4096."""
    _engine(monkeypatch, engine)
    gc = _grow(gpu_ctx, oracle, "fuzz_7_106_twice", {}, f"big[{engine}]")
    assert gc["rounds_big"] > 0, gc
    gc = _grow(gpu_ctx, oracle, "fuzz_7_106_twice", dict(max_waves=4096), f"big[{engine}]", unhooked_after=False)
    assert gc["rounds_big"] > 0 and gc["rounds_capped"] > 0 and gc["max_waves_end"] == 4096, gc


def test_cap_4096_equals_default_on_urban(gpu_ctx, oracle):
    """urban(400 000): attempts per round capped at 4096 and uncapped give the same bits (both the oracle's)."""
    _grow(gpu_ctx, oracle, "urban400k_k16", dict(max_waves=4096), "cap4096")
    _grow(gpu_ctx, oracle, "urban400k_k16", {}, "default")


# ---- 2. round pool ---------------------------------------------------------------------------------------------
# Pool capacities in int32 entries, found by scanning downwards from the default in steps of 1.5 and reading the
# counters (the default is max(64 n, 8 n + 6144 (n / 8 + 64)): 77.9 M entries for plane_cube).  (a): attempts end
# ST_NOMEM and the call succeeds; (b): smaller -- more of them, the attempts per round cut further.
POOL = {
    # (engine, input): ((a), (b))                       observed: attempts_nomem / waves_cut / max_waves_end / rounds
    ("v2", "plane_cube_k15"): (4264362, 1263514),     # (a) 30 / 3 / 24 / 4       (b) 2706 / 5 / 1 / 11
    ("v2", "facade400_k16"): (1348476, 898984),       # (a) 10 / 5 / 1 / 7        (b) 10 / 5 / 1 / 7
    ("v2", "urban400k_k16"): (5056789, 1498307),      # (a) 20 / 5 / 1 / 9        (b) 30 / 5 / 1 / 9
    ("v1", "plane_cube_k15"): (4264362, 1263514),     # (a) 463 / 3 / 24 / 6      (b) 3193 / 5 / 1 / 11
    ("v1", "facade400_k16"): (1348476, 898984),       # (a) 10 / 5 / 1 / 7        (b) 11 / 5 / 1 / 7
    ("v1", "urban400k_k16"): (5056789, 1498307),      # (a) 20 / 5 / 1 / 9        (b) 30 / 5 / 1 / 9
    ("k32", "plane_cube_k32"): (4264362, 2842908),    # (a) 710 / 4 / 3 / 6       (b) 1037 / 4 / 3 / 6
    ("k32", "boxes_k32"): (1933056, 169705),          # (a) 32 / 3 / 16 / 4       (b) 346 / 5 / 1 / 11
    ("v2", "tiny_tiles"): (1011168, 63198),           # (a) 3209 / 2 / 988 / 8    (b) 4521 / 4 / 15 / 129
    # One step (x 1.5) above (a) nothing runs out on the facade (2 022 715) and on urban (7 585 184); one step below (b)
    # the call ends BS_ERR_NOMEM: plane_cube k=15 842 342, k=32 1 895 272, facade 599 322, urban 998 871, boxes 113 136,
    # the tiles 987.  On these clouds the lowest open attempt soon IS the largest plane, the last to finish: a pool
    # that runs out for anybody runs out for it too, so (a) already cuts the attempts per round -- the regimes differ
    # in how many attempts run out and how far the cut goes, not in whether there is one.
}


@pytest.mark.parametrize("engine", ENGINES)
def test_round_pool_regime_a_some_attempts_run_out(gpu_ctx, oracle, monkeypatch, engine):
    _engine(monkeypatch, engine)
    for name in INPUTS[engine]:
        gc = _grow(gpu_ctx, oracle, name, dict(pool_cap=POOL[engine, name][0]), f"pool(a)[{engine}]")
        assert gc["attempts_nomem"] > 0 and gc["full_refreshes"] > 0, (name, gc)


@pytest.mark.parametrize("engine", ENGINES)
def test_round_pool_regime_b_the_lowest_attempt_runs_out(gpu_ctx, oracle, monkeypatch, engine):
    _engine(monkeypatch, engine)
    for name in INPUTS[engine]:
        gc = _grow(gpu_ctx, oracle, name, dict(pool_cap=POOL[engine, name][1]), f"pool(b)[{engine}]")
        assert gc["waves_cut"] > 0 and gc["attempts_nomem"] > 0 and gc["full_refreshes"] > 0, (name, gc)
        assert gc["max_waves_end"] < len(_input(oracle, name)[0]) // 8 + 64


@pytest.mark.parametrize("engine", ENGINES)
def test_round_pool_regime_c_too_small_for_the_largest_plane(gpu_ctx, oracle, monkeypatch, engine):
    """A pool of fewer int32 entries than the largest plane's list cannot hold that list: the call must end with
    BS_ERR_NOMEM (an ordinary status) after cutting the attempts per round down to one, and leave the context sound."""
    _engine(monkeypatch, engine)
    for name in INPUTS[engine]:
        xyz, normals, neigh, kw, want = _input(oracle, name)
        largest = int(np.diff(want[1]["offset"]).max())
        lim = dict(pool_cap=largest - 1)
        gpu_ctx.selftest_grow_limits(**lim)
        try:
            with pytest.raises(BsError) as e:
                gpu_ctx.region_grow(xyz, normals, neigh, api.default_params(k=neigh.shape[1], rg_mode=2, **kw))
            gc = gpu_ctx.grow_counters()
            _show(f"pool(c)[{engine}] {name}", lim, gc)
        finally:
            gpu_ctx.selftest_grow_limits()
        assert e.value.status == -3 and "round pool exhausted" in str(e.value)
        assert gc["max_waves_end"] == 1 and gc["attempts_nomem"] > 0 and gc["pool_cap"] == largest - 1
        _unhooked(gpu_ctx, oracle, name)


# ---- 3. pending room -------------------------------------------------------------------------------------------

_TILES = {}


def _tiles(O):
    if not _TILES:
        tiles = _tiny_tiles()
        p = api.default_params(k=15, th_point_count=100)
        _TILES["tiles"] = tiles
        _TILES["want"] = [_tile_oracle(O, x, p) for x in tiles]
        assert sum(len(w[3]) for w in _TILES["want"]) > 500  # (763 committed planes in 563 tiles)
    return _TILES["tiles"], _TILES["want"]


def _batch(ctx, O, lim, what):
    """segment_batch of the 2 000 tiny tiles (505 584 points) with the limits `lim`: every tile equal to the oracle."""
    tiles, want = _tiles(O)
    p = api.default_params(k=15, th_point_count=100, rg_mode=2)
    ctx.set_audit(True)
    try:
        ctx.selftest_grow_limits(**lim)
        out = ctx.segment_batch(tiles, p)
        gc = ctx.grow_counters()
        _show(f"{what} tiny_tiles", lim, gc)
        _audit_ok(ctx)
    finally:
        ctx.selftest_grow_limits()
        ctx.set_audit(False)
    for t in range(len(tiles)):
        _same(out[t], want[t], f"tile {t}")
    return gc


def _batch_unhooked(ctx, O):
    tiles, want = _tiles(O)
    out = ctx.segment_batch(tiles, api.default_params(k=15, th_point_count=100, rg_mode=2))
    gc = ctx.grow_counters()
    for t in range(len(tiles)):
        _same(out[t], want[t], f"tile {t} (no limits)")
    assert gc["dropped_pend_count"] == 0 and gc["dropped_pend_store"] == 0 and gc["attempts_nomem"] == 0, gc
    return gc


@pytest.mark.parametrize("max_pending", (1, 4, 64))
def test_pending_slots_run_out_in_a_batch(gpu_ctx, oracle, max_pending):
    """Many planes finish in one round of the batch; all but max_pending of those above the first open attempt are
    dropped from the structure and grown again."""
    gc = _batch(gpu_ctx, oracle, dict(max_pending=max_pending), "pending")
    assert gc["dropped_pend_count"] > 0 and gc["dropped_pend_store"] == 0
    _batch_unhooked(gpu_ctx, oracle)


def test_pending_store_runs_out_in_a_batch(gpu_ctx, oracle):
    gc = _batch(gpu_ctx, oracle, dict(pstore_cap=3000), "pstore")
    assert gc["dropped_pend_store"] > 0 and gc["dropped_pend_count"] == 0
    _batch_unhooked(gpu_ctx, oracle)


def test_capped_rounds_and_round_pool_in_a_batch(gpu_ctx, oracle):
    """The batch entry runs the same grower over the concatenation: capped rounds and an exhausted pool through it."""
    gc = _batch(gpu_ctx, oracle, dict(max_waves=64), "capped")
    assert gc["rounds_capped"] > 0
    for regime in (0, 1):
        gc = _batch(gpu_ctx, oracle, dict(pool_cap=POOL["v2", "tiny_tiles"][regime]), "pool(%s)" % "ab"[regime])
        assert gc["attempts_nomem"] > 0 and gc["waves_cut"] > 0 and gc["full_refreshes"] > 0, gc
    _batch_unhooked(gpu_ctx, oracle)


@pytest.mark.parametrize("lim", (dict(max_pending=1), dict(max_pending=4), dict(max_pending=64), dict(pstore_cap=3000)),
                         ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_pending_limits_on_urban_change_nothing(gpu_ctx, oracle, lim):
    """The same limits on one cloud, urban(400 000) with th_point_count = 0.  Measured: the cloud is done in ONE
    round in which every finished plane is final at once (no attempt below it stays open), so nothing ever waits
    for a pending slot there and neither drop counter can move -- this case only states that the lowered limits do
    not disturb such a run.  The counters are REQUIRED in the batch tests above and on the two inputs below."""
    gc = _grow(gpu_ctx, oracle, "urban400k_k16", lim, "pending")
    assert gc["dropped_pend_count"] == 0 and gc["dropped_pend_store"] == 0 and gc["rounds"] == 1, gc


@pytest.mark.parametrize("engine,name", (("v1", "fuzz_7_106"), ("v2", "fuzz_7_106"), ("k32", "fuzz_2718_16")))
@pytest.mark.parametrize("lim", (dict(max_pending=1), dict(pstore_cap=3000)), ids=("pending1", "pstore3000"))
def test_pending_room_on_every_engine(gpu_ctx, oracle, monkeypatch, engine, name, lim):
    """Pending room is a host-side path, but what is dropped is grown again by the engine: crossed on all three.
    (boxes() at k = 32 and plane_cube on the first engine cannot reach it -- measured: one round, every plane final at
    once, no drop with a limit of 1 -- so the inputs are the two fuzz clouds whose many small planes wait for each
    other: fuzz_2718_16 is k = 21, grow_spec_kernel<32>.)"""
    _engine(monkeypatch, engine)
    gc = _grow(gpu_ctx, oracle, name, lim, f"pending[{engine}]")
    assert gc["dropped_pend_count" if "max_pending" in lim else "dropped_pend_store"] > 0, gc


# ---- 4. re-growth policy ---------------------------------------------------------------------------------------

POLICIES = (("never", dict(retry_max_list=0)), ("short", dict(retry_max_list=1)), ("default", {}),
            ("always", dict(retry_big_round=0)))


@pytest.mark.parametrize("name,engines", (("fuzz_2718_16", ("k32",)), ("fuzz_7_106", ("v2", "v1")),
                                          ("plane_cube_k15", ("v2", "v1")), ("plane_cube_k32", ("k32",))))
def test_regrowth_policies_give_the_same_bits(gpu_ctx, oracle, monkeypatch, name, engines):
    """retry_max_list = 0 (a stolen plane always waits for the next round), 1, the default, and retry_big_round = 0
    (every round re-grows lists of any length inside the launch; MAX_RETRY / MAX_RETRY_LONG are the only brakes):
    all four are the oracle's bits.  fuzz_2718_16 (k = 21: grow_spec_kernel<32>) is the input of many small planes that
    kill and re-grow each other."""
    for engine in engines:
        _engine(monkeypatch, engine)
        stolen = {}
        for pol, lim in POLICIES:
            stolen[pol] = _grow(gpu_ctx, oracle, name, lim, f"policy[{engine}] {pol}", unhooked_after=False)["attempts_stolen"]
        if name.startswith("fuzz"):  # (rounds below 4096 attempts there: the host sees every stolen attempt)
            assert stolen["never"] > 0, stolen


def test_fuzz_with_random_limits():
    """The 40 fuzz cases of test_fuzz_negative_coordinates_and_noisy_normals, each with a random set of lowered
    limits (tests/tools/fuzz_parity.py --limits) and the audit replay."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "fuzz_parity.py"), "--cases", "40", "--seed", "4242",
                          "--audit", "--limits"], capture_output=True, text=True, timeout=900)
    print("\n".join(l for l in out.stdout.splitlines() if l.startswith(("limits reached", "done"))))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "40 cases, 0 mismatches" in out.stdout
    reached = dict(kv.split("=") for l in out.stdout.splitlines() if l.startswith("limits reached") for kv in l.split(": ")[1].split())
    assert int(reached["rounds_capped"]) > 0 and int(reached["full_refreshes"]) > 0, reached


# ---- 5. LIFO window --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine", ENGINES)
def test_lifo_window_is_crossed_many_times(gpu_ctx, oracle, monkeypatch, engine):
    """plane_cube's largest plane (62 501 entries) drives the LIFO of pending calls to tens of thousands of entries
    and back below the 256-entry LDS window hundreds of times -- stated by the oracle-side model (module docstring),
    so that a change of the input or of LDS_STACK cannot silently stop covering the spill / refill code -- and both
    grow modes equal the oracle."""
    _engine(monkeypatch, engine)
    name = "plane_cube_k32" if engine == "k32" else "plane_cube_k15"
    xyz, normals, neigh, kw, want = _input(oracle, name)
    sizes = np.diff(want[1]["offset"])
    peak, spills, refills, respills = (int(v) for v in want[2][int(sizes.argmax())])
    print(f"LIMITS lifo[{engine}] {name} | largest={int(sizes.max())} peak={peak} spills={spills} refills={refills} respills={respills}")
    assert sizes.max() == 62501
    assert peak >= 1024 and refills >= 8 and respills >= 8
    for mode in (1, 2):
        p = api.default_params(k=neigh.shape[1], rg_mode=mode, **kw)
        pi, planes = gpu_ctx.region_grow(xyz, normals, neigh, p)
        _equal_oracle(pi, planes, want)


# ---- 6. forced full refresh ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("plane_cube_k15", "urban400k_k16", "fuzz_2718_16", "fuzz_7_106"))
def test_full_refresh_every_round(gpu_ctx, oracle, name):
    """refresh_records_kernel before every round that grows something instead of the incremental records.  plane_cube
    and urban(400 000) are done in one round; the two fuzz clouds take 4 and ~1 040."""
    gc = _grow(gpu_ctx, oracle, name, dict(full_refresh=True), "refresh")
    assert gc["full_refreshes"] > 0
    assert gc["full_refreshes"] >= gc["rounds"] - 1  # (only a round with nothing but pending planes left grows nothing)


VERIFY_CHILD = r"""
import sys, json
import numpy as np
sys.path.insert(0, sys.argv[1])
from buildingsegment_amd import api, synth
sets = json.loads(sys.argv[2])
ctx = api.Context(0)
for name, xyz, k, kw in (("plane_cube_k15", synth.plane_cube(), 15, {}),
                         ("urban400k_k16", synth.urban(400_000, seed=9), 16, dict(th_point_count=0))):
    xyz = np.ascontiguousarray(xyz)
    for lim in sets[name]:
        ctx.selftest_grow_limits(**lim)
        neigh, normals, plane_idx, planes = ctx.segment(xyz, api.default_params(k=k, **kw))
        gc = ctx.grow_counters()
        print("RAN", name, json.dumps(lim), len(planes), gc["rounds"], gc["rounds_capped"], gc["attempts_nomem"], gc["full_refreshes"])
ctx.selftest_grow_limits()
"""


def test_self_checks_stay_silent_with_lowered_limits():
    """BS_VERIFY=1 (the owner structure is a fixed point of its equations after every settling; the incremental
    records equal a full refresh before every round) prints nothing with the limits of the tests above, the forced
    refresh included.  In a child process: the switch is read from the environment."""
    sets = {name: [dict(full_refresh=True), dict(max_waves=64), dict(pool_cap=POOL["v2", name][0]), dict(pool_cap=POOL["v2", name][1]),
                   dict(max_pending=1), dict(pstore_cap=3000)] for name in ("plane_cube_k15", "urban400k_k16")}
    out = subprocess.run([sys.executable, "-c", VERIFY_CHILD, ROOT, json.dumps(sets)], capture_output=True, text=True,
                         env=dict(os.environ, BS_VERIFY="1"), timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout)
    assert out.stdout.count("RAN") == 12
    assert "VERIFY:" not in out.stderr, out.stderr[-3000:]


# ---- 7. everything at once -------------------------------------------------------------------------------------

def test_everything_lowered_at_once(gpu_ctx, oracle):
    lim = dict(max_waves=64, pool_cap=POOL["v2", "urban400k_k16"][0], max_pending=4, retry_max_list=0)
    gc = _grow(gpu_ctx, oracle, "urban400k_k16", lim, "all")
    assert gc["rounds_capped"] > 0
    gc = _batch(gpu_ctx, oracle, dict(lim, pool_cap=POOL["v2", "tiny_tiles"][0]), "all")
    assert gc["rounds_capped"] > 0 and gc["dropped_pend_count"] > 0
    _batch_unhooked(gpu_ctx, oracle)


# ---- the hook itself -------------------------------------------------------------------------------------------

def test_hook_only_lowers_and_clears(gpu_ctx, oracle):
    """Capacities above the default are clamped to it; negative ones are refused; clearing restores the default."""
    n = len(_input(oracle, "plane_cube_k15")[0])
    default = _grow(gpu_ctx, oracle, "plane_cube_k15", {}, "default")
    big = dict(max_waves=1 << 30, pool_cap=1 << 40, max_pending=1 << 30, pstore_cap=1 << 40)
    gpu_ctx.selftest_grow_limits(**big)
    try:
        gpu_ctx.region_grow(*_input(oracle, "plane_cube_k15")[:3], api.default_params(k=15))
        gc = gpu_ctx.grow_counters()
    finally:
        gpu_ctx.selftest_grow_limits()
    assert gc["pool_cap"] == default["pool_cap"] >= 64 * n and gc["max_waves_end"] == default["max_waves_end"] == n // 8 + 64
    with pytest.raises(BsError) as e:
        gpu_ctx.selftest_grow_limits(pool_cap=-5)
    assert e.value.status == -1
    assert _unhooked(gpu_ctx, oracle, "plane_cube_k15")["pool_cap"] == default["pool_cap"]
