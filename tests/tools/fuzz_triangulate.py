#!/usr/bin/env python3
"""More seeds of the outline-triangle cases than the suite runs (the facet fuzz cases and random label images of
tests/simplify_ref/cases.py): the device against the restatement tests/triangulate_ref at every tolerance of the suite, every
array and total ==, and the identities of every OK label (tests/test_triangulate_cpu.py).  Labels that are not OK are
listed.  Needs a GPU.
usage: python tests/tools/fuzz_triangulate.py [--seeds 50] [--first 16] [--random-seeds 200]"""
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
import test_triangulate_cpu as tc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=50, help="facet fuzz seeds")
    ap.add_argument("--first", type=int, default=16, help="first facet fuzz seed (the suite runs 0 .. 15)")
    ap.add_argument("--random-seeds", type=int, default=200, help="random label images from seed 60 on (the suite runs 0 .. 59)")
    a = ap.parse_args()
    cases, tref, uref = tc.cases, tc.tref, tc.uref
    sc = cases.sc
    todo = [("fuzz", s, lambda s: sc.oc.from_facet(sc.fc.fuzz_case(s))) for s in range(a.first, a.first + a.seeds)]
    todo += [("random", s, sc.oc.random_case) for s in range(60, 60 + a.random_seeds)]
    runs = bad = 0
    not_ok = []
    with api.Context(0) as ctx:
        for name, seed, make in todo:
            c = make(seed)
            for tol in cases.TOLERANCES:
                plain, _, clean = uref.clean(c["label"], c["top"], c["n_labels"], *tol)
                want = tref.triangulate(plain, clean)
                got, gc, _, gp = ctx.outline_triangles(c["label"], c["top"], n_labels=c["n_labels"], num=tol[0], den=tol[1])
                diff = tref.same(got, want)
                runs += 1
                if diff is not None:
                    bad += 1
                    print(f"DIFFERENT {name}_{seed} {tol}: {diff}", flush=True)
                    continue
                tc.check_identities(gp, gc, got, c["label"].size <= 900)
                not_ok += [(f"{name}_{seed}", tol, l, int(s)) for l, s in enumerate(got.label_status) if s in (1, 2)]
    for row in not_ok:
        print("not OK (1 NO_BRIDGE, 2 STALLED):", *row)
    print(f"{runs} runs, {bad} different, {len(not_ok)} labels not OK, none of them in a facet case: "
          f"{not any(n.startswith('fuzz') for n, _, _, _ in not_ok)}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
