#!/usr/bin/env python3
"""More seeds of random label images through the clean outlines with sweeps (bs_set_outline_sweeps): the device against the
restatement tests/sweep_ref in modes 1 and 2 -- every array, total and sweep figure -- and the outcome after the repair: no
label without a bridge, none stalled, no pixel covered twice.  Exceptions are printed, one line each; the exit status is 1
where the device and the restatement differ.
usage: python tests/tools/fuzz_sweep.py [--seeds 200] [--first 1000] [--size 28]"""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from buildingsegment_amd import api  # noqa: E402

TOLERANCES = ((1, 1), (25, 4), (100, 1), (10 ** 6, 1))


def sweep_cases():
    spec = importlib.util.spec_from_file_location("sweep_cases", os.path.join(ROOT, "tests", "sweep_ref", "cases.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["sweep_cases"] = mod
    spec.loader.exec_module(mod)
    return mod


def image(seed, size):
    """blobs of a few labels with bays and islands: a smoothed noise field cut into labels, islands dropped in"""
    rng = np.random.default_rng(seed)
    h, w = rng.integers(size // 2, size + 1, 2)
    f = rng.random((h + 4, w + 4))
    for _ in range(int(rng.integers(1, 4))):
        f = (f + np.roll(f, 1, 0) + np.roll(f, -1, 0) + np.roll(f, 1, 1) + np.roll(f, -1, 1)) / 5
    f = f[2:-2, 2:-2]
    nl = int(rng.integers(1, 5))
    lab = np.digitize(f, np.quantile(f, np.linspace(0, 1, nl + 2)[1:-1])).astype(np.int32) - 1
    for _ in range(int(rng.integers(0, 6))):
        lab[rng.integers(0, h), rng.integers(0, w)] = rng.integers(-1, nl + 1)
    return lab, rng.integers(-500, 500, (h, w, 4)).astype(np.int32), nl + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=200)
    ap.add_argument("--first", type=int, default=1000)
    ap.add_argument("--size", type=int, default=28)
    a = ap.parse_args()
    cases = sweep_cases()
    wref, tbrute, boxwise = cases.wref, cases.tbrute, cases.boxwise
    ctx = api.Context(0)
    differ, exceptions, sweeping = 0, 0, 0
    for seed in range(a.first, a.first + a.seeds):
        lab, top, nl = image(seed, a.size)
        for tol in TOLERANCES:
            for mode in (1, 2):
                plain, _, want = wref.clean(lab, top, nl, *tol, mode=mode)
                got = ctx.clean_outlines(lab, top, n_labels=nl, num=tol[0], den=tol[1], sweeps=mode)[0]
                s = ctx.outline_sweeps()
                diff = wref.same(got, want, wref.DEVICE_FIELDS) or next(
                    (f for f in wref.SWEEP_FIELDS if getattr(s, f) != getattr(want, f)), None)
                if diff is not None:
                    differ += 1
                    print(f"DIFFERENT seed {seed} tol {tol} mode {mode}: {diff}", flush=True)
            sweeping += want.n_sweeping_first > 0
            if plain.n_rings:
                tri = tbrute.triangulate(plain, want)
                st = np.asarray(tri.label_status)
                failed = int(((st == tbrute.NO_BRIDGE) | (st == tbrute.STALLED)).sum())
                multi = int(boxwise.model_raster(want, tri, lab, top, nl).n_multi)
                if failed or multi:
                    exceptions += 1
                    print(f"EXCEPTION seed {seed} tol {tol}: failed labels {failed}, n_multi {multi}", flush=True)
    print(f"{a.seeds} seeds x {len(TOLERANCES)} tolerances: {sweeping} runs with a sweep, {differ} differences, "
          f"{exceptions} exceptions to the outcome")
    ctx.close()
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
