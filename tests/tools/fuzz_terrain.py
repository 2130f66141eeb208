#!/usr/bin/env python3
"""More seeds of the terrain stage than the suite runs: random building maps (boxes of random size, some touching the image's
edge or each other, up to --buildings of them) with a seeded cloud (a tilted sheet with holes, roof points, outliers below
it), random ring, quantile, min_ground and pixel edge: the device against the restatement tests/terrain_ref, every image and
figure ==, and on small images the brute force of the definition too.  Needs a GPU.
usage: python tests/tools/fuzz_terrain.py [--seeds 300] [--first 0] [--buildings 40]"""
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
import test_terrain_cpu as tc  # noqa: E402


def random_case(seed, max_buildings):
    rng = np.random.default_rng(31000 + seed)
    w, h = int(rng.integers(1, 120)), int(rng.integers(1, 90))
    bmap = np.full((h, w), -1, np.int32)
    nb = int(rng.integers(0, max_buildings + 1))
    for c in range(nb):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        bmap[y:y + int(rng.integers(1, 12)), x:x + int(rng.integers(1, 12))] = c
    bin_ = int(rng.choice([1, 7, 100, 500]))
    slope = int(rng.integers(-3, 4))
    holes = rng.random((h, w)) < rng.random() * 0.6
    xyz = tc.cases.sheet(bmap, bin_, seed, z_of=lambda x, y: slope * (x // max(bin_ // 10, 1)) - 40 * slope, per_pixel=int(rng.integers(1, 4)),
                         skip=holes, jitter=int(rng.integers(0, 30)))
    if len(xyz) == 0:
        xyz = np.zeros((1, 3), np.int32)
    low = xyz[rng.integers(0, len(xyz), max(len(xyz) // 50, 1))].copy()
    low[:, 2] -= rng.integers(1000, 9000, len(low)).astype(np.int32)
    q_den = int(rng.integers(1, 9))
    return tc.cases.case(f"random_{seed}", bmap, np.ascontiguousarray(np.concatenate([xyz, low])), ring=int(rng.integers(1, 40)), bin=bin_,
                         q=(int(rng.integers(0, q_den + 1)), q_den), min_ground=int(rng.integers(1, 12)),
                         fallback_z=int(rng.integers(-5000, 5000)), n_buildings=nb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=300)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--buildings", type=int, default=40)
    a = ap.parse_args()
    tref, brute = tc.tref, tc.brute
    runs = bad = fallbacks = 0
    with api.Context(0) as ctx:
        for seed in range(a.first, a.first + a.seeds):
            c = random_case(seed, a.buildings)
            got = ctx.terrain(c["xyz"], c["bmap"], c["n_buildings"], bin=c["bin"], ring=c["ring"], q=c["q"], min_ground=c["min_ground"],
                              fallback_z=c["fallback_z"])
            want = tref.terrain(*tc.cases.args(c))
            diff = tref.same(got, want)
            if diff is None and c["bmap"].size <= 1500:
                diff = brute.same(got, brute.terrain(*tc.cases.args(c)))
            runs += 1
            fallbacks += got.n_fallback
            if diff is not None:
                bad += 1
                print(f"DIFFERENT random_{seed}: {diff}", flush=True)
    print(f"{runs} runs, {bad} different, {fallbacks} buildings on the fallback")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
