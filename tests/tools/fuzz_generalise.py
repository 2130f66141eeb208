#!/usr/bin/env python3
"""More seeds of the roof-generalisation fuzz cases than the suite runs (tests/generalise_ref/cases.py): the device
against the restatement, every array ==, and the converged output run again (idempotence).  Needs a GPU, except --search,
which looks through the seeds on the CPU for the regimes the suite names by seed (SEED_WAITS, SEED_THREE_ROUNDS,
SEED_FLAT_LATER).
usage: python tests/tools/fuzz_generalise.py [--seeds 300] [--first 28] [--small-seeds 0] | --search [--seeds 60]"""
import argparse
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def load_cases():
    spec = importlib.util.spec_from_file_location("generalise_cases", os.path.join(ROOT, "tests", "generalise_ref", "cases.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["generalise_cases"] = mod
    spec.loader.exec_module(mod)
    return mod


def search(cases, seeds):
    found = {}
    for s in range(seeds):
        c = cases.fuzz_case(s)
        ref = cases.run_ref(c)
        for k in {"waits_then_moves", "three_rounds", "flat_only_later"} & cases.regimes(c, ref):
            found.setdefault(k, []).append((s, ref.rounds))
    for k, v in sorted(found.items()):
        print(k, v)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=300)
    ap.add_argument("--first", type=int, default=None, help="first seed (the suite runs 0 .. N_FUZZ - 1)")
    ap.add_argument("--small-seeds", type=int, default=0, help="also this many seeds of the small cases")
    ap.add_argument("--search", action="store_true")
    a = ap.parse_args()
    cases = load_cases()
    if a.search:
        return search(cases, a.seeds)
    import torch
    torch.zeros(1, device="cuda")
    from buildingsegment_amd import api
    first = cases.N_FUZZ if a.first is None else a.first
    todo = [("fuzz", s, cases.fuzz_case) for s in range(first, first + a.seeds)]
    todo += [("small", s, cases.small_case) for s in range(a.small_seeds)]
    bad = 0
    with api.Context(0) as ctx:
        def run(c):
            roofs = SimpleNamespace(roof=c["roof"], normal=c["normal"], center=c["center"], z_min=c["z_min"], z_max=c["z_max"],
                                    bin=c["bin"])
            return ctx.generalise_roofs(c["bmap"], roofs, base_z=c["base_z"], flat=c["flat"], **c["params"])

        for name, seed, make in todo:
            c = make(seed)
            got = run(c)
            diff = cases.gr.same(got, cases.run_ref(c))
            if diff is None and got.converged:
                again = run(dict(c, roof=got.roof))
                if again.rounds != 0 or not np.array_equal(again.roof, got.roof):
                    diff = "idempotence"
            if diff is not None:
                bad += 1
                print(f"{name} seed {seed}: differs in {diff}", flush=True)
    print(f"{len(todo)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
