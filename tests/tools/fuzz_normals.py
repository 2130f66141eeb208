#!/usr/bin/env python3
"""More seeds of the neighbourhood families of tests/normal_ref/cases.py than the suite runs.

Per seed: 36 clusters of every family, placed as the 'near' and the 'domain' cloud.  On the CPU: the traced restatement
(tests/normal_ref/trace.py) against oracle.fast_eigen3x3 and oracle.normal_from_list bit for bit, norm and orientation
of every result, and the count of every leaf the seed reaches (a leaf outside cases.REQUIRED is reported: it belongs
into the list).  With --gpu (MI355X box): both clouds through bs_knn_normals with relative 32-bit and absolute 64-bit
moments and through bs_plane_fit -- rows and 64-bit patterns against the oracle, one normal per cluster, no query
work-listed.  Every comparison is ==.
usage: python tests/tools/fuzz_normals.py [--seeds N] [--seed S] [--gpu]
"""
import argparse
import collections
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "fit_ref"))

from normal_ref import cases, trace  # noqa: E402
from oracle import oracle as O  # noqa: E402

PER_FAMILY = 36  # 11 families: 396 of the 405 slots


def run_seed(seed, ctx=None):
    rng = np.random.default_rng(seed)
    clusters = cases.draw_list(rng, PER_FAMILY)
    seen, bad = collections.Counter(), 0
    for where in ("near", "domain"):
        for i, c in enumerate(clusters):
            pts = cases.placed(c, i, cases.PITCH, where)
            c6 = trace.cov_of(pts.tolist())
            v, lv = trace.fast_eigen3x3(c6)
            tail, _ = trace.normal_of_cov(c6)
            n = O.normal_from_list(pts.astype(np.int32), np.arange(len(pts), dtype=np.int32))
            ok = (np.array_equal(trace.bits(v), trace.bits(O.fast_eigen3x3(c6))) and np.array_equal(trace.bits(tail), trace.bits(n)))
            if ok and not np.isnan(n).any():
                ok = abs(math.sqrt(float(n @ n)) - 1) < 1e-12 and n[2] >= 0
            if not ok:
                bad += 1
                print(f"seed {seed} {where} {c['name']}: MISMATCH leaves {lv}\n  points {pts.tolist()}")
            seen.update(set(lv))
        if ctx is not None:
            bad += run_gpu(ctx, seed, where, *cases.cloud(clusters, cases.PITCH, where))
    return seen, bad


def run_gpu(ctx, seed, where, xyz, cid, sizes):
    from buildingsegment_amd import api
    import fit_ref as fr
    bad = 0
    p = api.default_params(k=3, radius=cases.RADIUS, max_nn=64)
    oneigh, onormals = O.knn_normals(xyz, k=3, radius=cases.RADIUS, max_nn=64)
    first = np.full(len(sizes), -1)
    first[cid[::-1]] = np.arange(len(cid))[::-1]
    for name in (None, "BS_KNN_MOMENTS64"):
        os.environ.pop("BS_KNN_MOMENTS64", None)
        if name:
            os.environ[name] = "1"
        neigh, normals = ctx.knn_normals(xyz, p)
        fb = ctx.timings()["n_fallback_queries"]
        bits = normals.view(np.int64)
        diff = (bits != onormals.view(np.int64)).any(axis=1)
        split = (bits != bits[first[cid]]).any(axis=1)
        if not np.array_equal(neigh, oneigh) or diff.any() or split.any() or fb:
            bad += 1
            print(f"seed {seed} {where} {name or 'REL32'}: rows differ {(neigh != oneigh).any(axis=1).sum()}, normals differ in "
                  f"clusters {np.unique(cid[diff])[:8]}, clusters not of one normal {np.unique(cid[split])[:8]}, work-listed {fb}")
    os.environ.pop("BS_KNN_MOMENTS64", None)
    lab = (cid + 1).astype(np.int32)
    got, ref = ctx.plane_fit(xyz, lab, len(sizes)), fr.plane_fit(xyz, lab, len(sizes))
    diff = (got.normal.view(np.int64) != ref.normal.view(np.int64)).any(axis=1)
    if diff.any():
        bad += 1
        print(f"seed {seed} {where} plane fit: normals of clusters {np.nonzero(diff)[0][:8]} differ")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--gpu", action="store_true")
    a = ap.parse_args()
    ctx = None
    if a.gpu:
        from buildingsegment_amd import api
        ctx = api.Context(0)
    total, bad, t0 = collections.Counter(), 0, time.time()
    for s in range(a.seed, a.seed + a.seeds):
        seen, b = run_seed(s, ctx)
        total.update(seen)
        bad += b
    print("leaf      placed clusters")
    for l in trace.LEAVES:
        print("%-8s %7d%s" % (l, total[l], "" if l in cases.REQUIRED else ("   NOT IN REQUIRED" if total[l] else "   (not required)")))
    print(f"{a.seeds} seeds, {bad} mismatches, {time.time() - t0:.1f} s")
    if ctx is not None:
        ctx.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
