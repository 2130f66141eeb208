#!/usr/bin/env python3
"""More seeds of the roof-facet fuzz cases than the suite runs (tests/facet_ref/cases.py): the device against the
restatement, every array ==.  Needs a GPU.
usage: python tests/tools/fuzz_facets.py --facets [--seeds 200] [--first 16] [--solid-seeds 0]"""
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
    spec = importlib.util.spec_from_file_location("facet_cases", os.path.join(ROOT, "tests", "facet_ref", "cases.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["facet_cases"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--facets", action="store_true", help="run the roof-facet cases (the only stage of this tool)")
    ap.add_argument("--seeds", type=int, default=200)
    ap.add_argument("--first", type=int, default=16, help="first seed (the suite runs 0 .. 15)")
    ap.add_argument("--solid-seeds", type=int, default=0, help="also this many seeds of the solid fuzz cases from 40 on")
    a = ap.parse_args()
    if not a.facets:
        ap.error("nothing to do: give --facets")
    cases = load_cases()
    todo = [("fuzz", s, cases.fuzz_case) for s in range(a.first, a.first + a.seeds)]
    todo += [("solid_fuzz", s, cases.solid_fuzz_case) for s in range(40, 40 + a.solid_seeds)]
    bad = 0
    with api.Context(0) as ctx:
        for name, seed, make in todo:
            c = make(seed)
            got = ctx.roof_facets(c["bmap"], c["roof"], c["top"], n_buildings=c["n_buildings"], n_planes=c["n_planes"])
            diff = cases.fr.same(got, cases.run_ref(c))
            if diff is not None:
                bad += 1
                print(f"{name} seed {seed}: differs in {diff}", flush=True)
    print(f"{len(todo)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
