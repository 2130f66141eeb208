#!/usr/bin/env python3
"""More seeds of the simplified-outline cases than the suite runs (tests/simplify_ref/cases.py): the device against the
restatement at every tolerance of the suite, with top and without, every array and total ==.  Needs a GPU.
usage: python tests/tools/fuzz_simplify.py [--seeds 100] [--first 16] [--random-seeds 200]"""
import argparse
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
torch.zeros(1, device="cuda")
from buildingsegment_amd import api  # noqa: E402


def load_cases():
    spec = importlib.util.spec_from_file_location("simplify_cases", os.path.join(ROOT, "tests", "simplify_ref", "cases.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["simplify_cases"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=100, help="facet fuzz seeds")
    ap.add_argument("--first", type=int, default=16, help="first facet fuzz seed (the suite runs 0 .. 15)")
    ap.add_argument("--random-seeds", type=int, default=200, help="random label images from seed 60 on (the suite runs 0 .. 59)")
    a = ap.parse_args()
    cases = load_cases()
    oc, fc, sref = cases.oc, cases.fc, cases.sref
    todo = [("fuzz", s, lambda s: oc.from_facet(fc.fuzz_case(s))) for s in range(a.first, a.first + a.seeds)]
    todo += [("random", s, oc.random_case) for s in range(60, 60 + a.random_seeds)]
    runs = bad = 0
    with api.Context(0) as ctx:
        for name, seed, make in todo:
            c = make(seed)
            for tol in cases.TOLERANCES:
                _, want = cases.run_ref(c, tol)
                runs += 1
                for top in (c["top"], None):
                    got, _ = ctx.simplified_outlines(c["label"], top, n_labels=c["n_labels"], num=tol[0], den=tol[1])
                    if top is None:
                        got.sz = want.sz
                    diff = sref.same(got, want)
                    if diff is not None:
                        bad += 1
                        print(f"{name} seed {seed} tolerance {tol} top {top is not None}: differs in {diff}", flush=True)
    print(f"{len(todo)} cases, {runs} runs, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
