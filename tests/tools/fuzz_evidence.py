#!/usr/bin/env python3
"""More seeds of the roof evidence than the suite runs: random lattices (some narrower than the window, some one tile wide
and hundreds of pixels long, some of more tiles than one sweep of the window kernel), random fill, labels, plane tables,
radius, min_points and share, every fourth cloud in scan order (sorted by pixel), some of more points than one sweep of the
counts pass, with and without a ground model: the device against the restatement tests/evidence_ref, every
image and figure ==, and below 1 500 pixels the brute force of the definition too.  Every third seed also runs
bs_footprints under the keep image against tests/footprint_ref on the AND-ed mask.  Needs a GPU.
usage: python tests/tools/fuzz_evidence.py [--seeds 300] [--first 0]"""
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
import test_evidence_cpu as tc  # noqa: E402

FIELDS = ("width", "height") + tc.eref.FIGURES


def random_case(seed):
    rng = np.random.default_rng(83000 + seed)
    shape = rng.integers(0, 10)
    w, h = int(rng.integers(2, 120)), int(rng.integers(2, 90))
    if shape == 0:
        w, h = int(rng.integers(300, 1500)), int(rng.integers(2, 5))
    elif shape == 1:
        w, h = int(rng.integers(2, 5)), int(rng.integers(300, 1500))
    elif shape == 2:
        w, h = int(rng.integers(500, 800)), int(rng.integers(500, 800))  # more tiles than one sweep
    elif shape == 3:
        w, h = int(rng.integers(2, 40)), int(rng.integers(2, 38))        # small enough for the brute force
    n_planes = int(rng.integers(0, 9))
    ok = None if rng.random() < 0.2 else (rng.random(n_planes) < 0.6).astype(np.uint8)
    den = int(rng.integers(1, 9))
    n = int(rng.integers(1, 4 * w * h + 2)) if w * h < 20000 else int(rng.integers(1, 400000))
    if shape == 4:
        n = int(rng.integers(tc.cases.SWEEP + 1, tc.cases.SWEEP + 200000))  # a second point for some threads
    scan = int(rng.integers(1, n + 1)) if seed % 4 == 1 else 0
    model = tc.cases.tilted_model(w, h, int(rng.choice([150, 200, 500]))) if rng.random() < 0.3 else None
    return tc.cases.noise(f"random_{seed}", w, h, n, 83000 + seed, r=int(rng.integers(0, 16)), min_points=int(rng.integers(1, 12)),
                          share=(int(rng.integers(0, den + 1)), den), n_planes=n_planes, ok=ok, fill=float(rng.random()),
                          bin=int(rng.choice([1, 7, 100])) if model is None else 100, ground_th=float(rng.integers(0, 3000)), model=model,
                          scan_tail=scan)


def screen_differs(ctx, keep, rng):
    """bs_footprints under `keep` against the restatement on the AND-ed mask"""
    h, w = keep.shape
    img = np.zeros((h, w, 3))
    img[..., 1] = np.where(rng.random((h, w)) < 0.6, rng.uniform(1.0, 30.0, (h, w)), 0.0)
    ctx.set_footprint_screen(keep)
    try:
        fp, mask = ctx.footprints(img, return_mask=True)
    finally:
        ctx.set_footprint_screen(None)
    want, want_mask = tc.eref.screened_footprints(img, keep)
    if not np.array_equal(mask, want_mask * 255):
        return "screened mask"
    if len(fp.contours) != len(want.contours) or not all(np.array_equal(a, b) for a, b in zip(fp.contours, want.contours)):
        return "screened contours"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=300)
    ap.add_argument("--first", type=int, default=0)
    a = ap.parse_args()
    eref, brute = tc.eref, tc.brute
    runs = bad = brutes = screens = 0
    with api.Context(0) as ctx:
        for seed in range(a.first, a.first + a.seeds):
            c = random_case(seed)
            ctx.set_ground_model(*(c["model"] if c["model"] is not None else (None,)))
            got = ctx.roof_evidence(c["xyz"], c["plane_idx"], c["n_planes"], c["plane_ok"], c["extent"], c["bin"], c["ground_th"],
                                    c["params"])
            ctx.set_ground_model(None)
            want = eref.evidence(*tc.cases.args(c))
            diff = next((k for k in FIELDS if getattr(got, k) != getattr(want, k)), None)
            diff = diff or next((k for k in eref.IMAGES if not np.array_equal(getattr(got, k), getattr(want, k))), None)
            if diff is None and want.width * want.height < 1500:
                diff = eref.same(want, brute.evidence(*tc.cases.args(c)))
                brutes += 1
            if diff is None and seed % 3 == 0 and want.width * want.height < 200000:
                diff = screen_differs(ctx, got.keep, np.random.default_rng(seed))
                screens += 1
            runs += 1
            if diff is not None:
                bad += 1
                print(f"DIFFERENT random_{seed}: {diff} ({want.width} x {want.height}, {c['params']})", flush=True)
    print(f"{runs} runs ({brutes} also against the brute force, {screens} also through the screened footprints), {bad} different")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
