#!/usr/bin/env python3
"""More seeds of the facet-outline cases than the suite runs (tests/outline_ref/cases.py): the device against the
restatement, with top and without, every array ==.  Needs a GPU.
usage: python tests/tools/fuzz_outlines.py [--seeds 200] [--first 16] [--solid-seeds 0] [--random-seeds 0]"""
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
    spec = importlib.util.spec_from_file_location("outline_cases", os.path.join(ROOT, "tests", "outline_ref", "cases.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["outline_cases"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=200, help="facet fuzz seeds")
    ap.add_argument("--first", type=int, default=16, help="first facet fuzz seed (the suite runs 0 .. 15)")
    ap.add_argument("--solid-seeds", type=int, default=0, help="also this many seeds of the solid fuzz cases from 40 on")
    ap.add_argument("--random-seeds", type=int, default=0, help="also this many random label images from seed 60 on")
    a = ap.parse_args()
    cases = load_cases()
    fc, orf = cases.fc, cases.orf
    todo = [("fuzz", s, lambda s: cases.from_facet(fc.fuzz_case(s))) for s in range(a.first, a.first + a.seeds)]
    todo += [("solid_fuzz", s, lambda s: cases.from_facet(fc.solid_fuzz_case(s))) for s in range(40, 40 + a.solid_seeds)]
    todo += [("random", s, cases.random_case) for s in range(60, 60 + a.random_seeds)]
    bad = 0
    with api.Context(0) as ctx:
        for name, seed, make in todo:
            c = make(seed)
            want = cases.run_ref(c)
            got = ctx.facet_outlines(c["label"], c["top"], n_labels=c["n_labels"])
            flat = ctx.facet_outlines(c["label"], None, n_labels=c["n_labels"])
            diff = orf.same(got, want)
            if diff is None and flat.z is None:
                flat.z = want.z
                diff = orf.same(flat, want)
            if diff is not None:
                bad += 1
                print(f"{name} seed {seed}: differs in {diff}", flush=True)
    print(f"{len(todo)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
