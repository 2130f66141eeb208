#!/usr/bin/env python3
"""More seeds of the ground stage than the suite runs: random lattices (some one pixel wide or high in points, some longer
than a row segment of the x passes), a rough tilted sheet with boxes, holes of EMPTY pixels and points far below the sheet,
random radii, slope, thresholds and cell: the device against the restatement tests/ground_ref, every array and figure ==, and
on small lattices the brute force of the definition too.  Needs a GPU.
usage: python tests/tools/fuzz_ground.py [--seeds 300] [--first 0]"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.zeros(1, device="cuda")
from buildingsegment_amd import api  # noqa: E402
import test_ground_cpu as tc  # noqa: E402

FIELDS = ("width", "height", "threshold", "step_pixels") + tc.gref.FIGURES


def random_case(seed):
    rng = np.random.default_rng(47000 + seed)
    shape = rng.integers(0, 10)
    w, h = int(rng.integers(2, 160)), int(rng.integers(2, 110))
    if shape == 0:
        w, h = int(rng.integers(1500, 4500)), int(rng.integers(2, 5))  # more than one row segment
    elif shape == 1:
        w, h = int(rng.integers(2, 5)), int(rng.integers(300, 1500))
    cell = int(rng.choice([1, 7, 100, 500]))
    low = tc.cases.relief(w, h, seed, boxes=int(rng.integers(0, 8)), amp=int(rng.integers(0, 400)))
    low[rng.random((h, w)) < rng.random() * 0.5] = tc.EMPTY
    if rng.random() < 0.5:  # a hole
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        low[y:y + int(rng.integers(1, 60)), x:x + int(rng.integers(1, 60))] = tc.EMPTY
    if (low == tc.EMPTY).all():
        low[0, 0] = 0
    pits = (rng.random((h, w)) < 0.01) & (low != tc.EMPTY)
    low[pits] -= rng.integers(1000, 9000, int(pits.sum()))
    k = int(rng.integers(1, 7))
    radius = np.sort(rng.choice(np.arange(1, 256 if rng.random() < 0.2 else 40), size=k, replace=False)).tolist()
    return tc.cases.case(f"random_{seed}", low, cell, seed, extra=int(rng.integers(0, 3)), radius=radius,
                         slope=(int(rng.integers(0, 12)), int(rng.integers(1, 12))), dh0=int(rng.integers(0, 400)),
                         dh_max=int(rng.integers(0, 3000)), tol=int(rng.integers(0, 400)), min_height=int(rng.integers(0, 3000)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=300)
    ap.add_argument("--first", type=int, default=0)
    a = ap.parse_args()
    gref, brute = tc.gref, tc.brute
    runs = bad = 0
    with api.Context(0) as ctx:
        for seed in range(a.first, a.first + a.seeds):
            c = random_case(seed)
            got = ctx.ground(*tc.cases.args(c))
            want = gref.ground(*tc.cases.args(c))
            diff = next((k for k in FIELDS if getattr(got, k) != getattr(want, k)), None)
            diff = diff or next((k for k in ("low", "dtm", "step", "hag", "cls") if not np.array_equal(getattr(got, k), getattr(want, k))), None)
            if diff is None and want.width * want.height <= 1500 and max(c["params"]["radius"]) <= 12:
                diff = gref.same(want, brute.ground(*tc.cases.args(c)))
            runs += 1
            if diff is not None:
                bad += 1
                print(f"DIFFERENT random_{seed}: {diff} ({want.width} x {want.height}, radii {c['params']['radius']})", flush=True)
    print(f"{runs} runs, {bad} different")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
