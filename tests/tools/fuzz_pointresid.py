#!/usr/bin/env python3
"""More seeds of the point-residual cases than the suite runs (the facet fuzz cases and random label images of
tests/simplify_ref/cases.py, each with the seeded cloud of tests/pointresid_ref/cases.py at every pixel edge of its BINS): the
device against the restatement tests/pointresid_ref over the device's own clean outlines and triangles at every tolerance of
the suite, every per-point value and figure ==, and the first three promises.  Runs with points covered twice are listed.
Needs a GPU.
usage: python tests/tools/fuzz_pointresid.py [--seeds 50] [--first 16] [--random-seeds 200]"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.zeros(1, device="cuda")
from buildingsegment_amd import api  # noqa: E402
import test_pointresid_cpu as pc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=50, help="facet fuzz seeds")
    ap.add_argument("--first", type=int, default=16, help="first facet fuzz seed (the suite runs 0 .. 15)")
    ap.add_argument("--random-seeds", type=int, default=200, help="random label images from seed 60 on (the suite runs 0 .. 59)")
    a = ap.parse_args()
    cases, pref, brute = pc.cases, pc.pref, pc.brute
    sc = cases.sc
    todo = [("fuzz", s, lambda s: sc.oc.from_facet(sc.fc.fuzz_case(s))) for s in range(a.first, a.first + a.seeds)]
    todo += [("random", s, sc.oc.random_case) for s in range(60, 60 + a.random_seeds)]
    runs = bad = 0
    twice = []
    with api.Context(0) as ctx:
        for name, seed, make in todo:
            c = make(seed)
            h, w = c["label"].shape
            for tol in cases.tc.TOLERANCES:
                gt, gc, _, _ = ctx.outline_triangles(c["label"], c["top"], n_labels=c["n_labels"], num=tol[0], den=tol[1])
                b = cases.BINS[(seed + tol[0]) % len(cases.BINS)]
                k = cases.cloud(f"{name}_{seed}", c, tol, b, gc, gt)
                got = ctx.point_residuals(c["label"], c["top"], k.xyz, n_labels=c["n_labels"], num=tol[0], den=tol[1], bin=b,
                                          plane_idx=k.plane_idx, label_plane=k.label_plane, clip2=k.clip2)[0]
                want = pref.point_residuals(gc, gt, c["n_labels"], w, h, k.xyz, b, k.plane_idx, k.label_plane, k.clip2)
                diff = pref.same(got, want)
                runs += 1
                if diff is not None:
                    bad += 1
                    print(f"DIFFERENT {name}_{seed} {tol} bin {b}: {diff}", flush=True)
                    continue
                brute.check_promises(got, c["label"], gt.label_status, tolerance_zero=tol[0] == 0, xyz=k.xyz)
                if got.n_multi:
                    twice.append((f"{name}_{seed}", tol, b, got.n_multi))
    for row in twice:
        print("points covered twice:", *row)
    print(f"{runs} runs, {bad} different, {len(twice)} with points covered twice")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
