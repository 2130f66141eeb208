#!/usr/bin/env python3
"""More seeds of the model-raster cases than the suite runs (the facet fuzz cases and random label images of
tests/simplify_ref/cases.py): the device against the restatement tests/modelraster_ref over the device's own clean outlines
and triangles at every tolerance of the suite, every image and figure ==, and the three promises.  Runs with pixels covered
twice are listed.  Needs a GPU.
usage: python tests/tools/fuzz_modelraster.py [--seeds 50] [--first 16] [--random-seeds 200]"""
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
import test_modelraster_cpu as mc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=50, help="facet fuzz seeds")
    ap.add_argument("--first", type=int, default=16, help="first facet fuzz seed (the suite runs 0 .. 15)")
    ap.add_argument("--random-seeds", type=int, default=200, help="random label images from seed 60 on (the suite runs 0 .. 59)")
    a = ap.parse_args()
    cases, mref, brute = mc.cases, mc.mref, mc.brute
    sc = cases.sc
    todo = [("fuzz", s, lambda s: sc.oc.from_facet(sc.fc.fuzz_case(s))) for s in range(a.first, a.first + a.seeds)]
    todo += [("random", s, sc.oc.random_case) for s in range(60, 60 + a.random_seeds)]
    runs = bad = 0
    twice = []
    with api.Context(0) as ctx:
        for name, seed, make in todo:
            c = make(seed)
            for tol in cases.tc.TOLERANCES:
                got, gt, gc, _, _ = ctx.model_raster(c["label"], c["top"], n_labels=c["n_labels"], num=tol[0], den=tol[1])
                want = mref.model_raster(gc, gt, c["label"], c["top"], c["n_labels"])
                diff = mref.same(got, want)
                runs += 1
                if diff is not None:
                    bad += 1
                    print(f"DIFFERENT {name}_{seed} {tol}: {diff}", flush=True)
                    continue
                brute.check_promises(got, c["label"], gt.label_status, tolerance_zero=tol[0] == 0)
                if got.n_multi:
                    twice.append((f"{name}_{seed}", tol, got.n_multi))
    for row in twice:
        print("pixels covered twice:", *row)
    print(f"{runs} runs, {bad} different, {len(twice)} with pixels covered twice")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
