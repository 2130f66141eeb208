#!/usr/bin/env python3
"""More seeds of the oriented-box fuzz cases than the suite runs (tests/hull_ref/cases.py: the random label images of the
outline suite and the facet fuzz images): the device against the definition in Python integers, every array ==, and the
layout figures against the restatement.  Needs a GPU.
usage: python tests/tools/fuzz_hulls.py [--seeds 200] [--first 60] [--facet-seeds 0]"""
import argparse
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
torch.zeros(1, device="cuda")
from buildingsegment_amd import api, hulls  # noqa: E402


def load_cases():
    spec = importlib.util.spec_from_file_location("hull_cases", os.path.join(ROOT, "tests", "hull_ref", "cases.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["hull_cases"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=200, help="random label images")
    ap.add_argument("--first", type=int, default=60, help="first random seed (the suite runs 0 .. 59)")
    ap.add_argument("--facet-seeds", type=int, default=0, help="also this many facet fuzz images from seed 16 on")
    a = ap.parse_args()
    cases = load_cases()
    oc, fc = cases.oc, cases.fc
    todo = [("random", s, oc.random_case) for s in range(a.first, a.first + a.seeds)]
    todo += [("facet_fuzz", s, lambda s: oc.from_facet(fc.fuzz_case(s))) for s in range(16, 16 + a.facet_seeds)]
    bad = 0
    with api.Context(0) as ctx:
        for name, seed, make in todo:
            o = make(seed)
            c = cases.case(o["label"], o["n_labels"])
            got = hulls.label_hulls(ctx, *c)
            diff = cases.brute.same(got, cases.run_brute(c))
            if diff is None and {k: got.info[k] for k in ("n_candidates", "rounds", "max_live")} != cases.run_ref(c).info:
                diff = "layout figures"
            if diff is not None:
                bad += 1
                print(f"{name} seed {seed}: differs in {diff}", flush=True)
    print(f"{len(todo)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
