#!/usr/bin/env python3
"""More seeds of the oriented-box fuzz cases than the suite runs (tests/hull_ref/cases.py: the random label images of the
outline suite and the facet fuzz images): the device against the definition in Python integers, every array ==, and the
layout figures against the restatement.  Needs a GPU.
With --cases it runs the sparse generator instead (cases.sparse_fuzz: 1 to 3 labels of 3 to 40 single pixels in an image whose
sides lie within 3 of 1150, 2048, 4096 or, one axis at a time, the bound of 16383; the suite runs seeds 0 .. 19): without
--gpu the definition against the restatement on the CPU, with --gpu the device against both.
usage: python tests/tools/fuzz_hulls.py [--seeds 200] [--first 60] [--facet-seeds 0]
       python tests/tools/fuzz_hulls.py --cases 500 [--seed 20] [--gpu]"""
import argparse
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
LAYOUT = ("n_candidates", "rounds", "max_live")


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
    ap.add_argument("--cases", type=int, default=0, help="this many sparse cases instead")
    ap.add_argument("--seed", type=int, default=20, help="first seed of the sparse cases (the suite runs 0 .. 19)")
    ap.add_argument("--gpu", action="store_true", help="sparse cases on the device too")
    a = ap.parse_args()
    cases = load_cases()
    if a.cases and not a.gpu:
        bad = 0
        for seed in range(a.seed, a.seed + a.cases):
            s = cases.sparse_fuzz(seed)
            diff = cases.brute.same(cases.sparse_brute(s), cases.sparse_ref(s))
            if diff is not None:
                bad += 1
                print(f"sparse seed {seed}: the restatement differs in {diff}", flush=True)
        print(f"{a.cases} cases, {bad} differ")
        return 1 if bad else 0
    import torch
    torch.zeros(1, device="cuda")
    from buildingsegment_amd import api, hulls
    oc, fc = cases.oc, cases.fc
    todo = [("random", s, oc.random_case) for s in range(a.first, a.first + a.seeds)]
    todo += [("facet_fuzz", s, lambda s: oc.from_facet(fc.fuzz_case(s))) for s in range(16, 16 + a.facet_seeds)]
    if a.cases:
        todo = [("sparse", s, cases.sparse_fuzz) for s in range(a.seed, a.seed + a.cases)]
    bad = 0
    with api.Context(0) as ctx:
        for name, seed, make in todo:
            o = make(seed)
            if name == "sparse":
                c, want, ref = cases.dense(o), cases.sparse_brute(o), cases.sparse_ref(o)
            else:
                c = cases.case(o["label"], o["n_labels"])
                want, ref = cases.run_brute(c), cases.run_ref(c)
            got = hulls.label_hulls(ctx, *c)
            diff = cases.brute.same(got, want)
            if diff is None and {k: got.info[k] for k in LAYOUT} != ref.info:
                diff = "layout figures"
            if diff is not None:
                bad += 1
                print(f"{name} seed {seed}: differs in {diff}", flush=True)
    print(f"{len(todo)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
