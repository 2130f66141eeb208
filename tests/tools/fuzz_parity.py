#!/usr/bin/env python3
"""Differential fuzzing of the HIP path against the CPU oracle (GPU box only).

Random small clouds (surfaces, blobs, lattices with heavy ties), random k,
thresholds, normal noise and point orders; every stage is compared bit for bit
(neighbour indices, normals, labels, plane lists) in both region-grow modes.
usage: python tests/tools/fuzz_parity.py [--cases N] [--seed S] [--log FILE] [--audit] [--limits]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make_case(rng):
    kind = rng.integers(0, 5)
    n = int(rng.integers(300, 30000))
    if kind == 0:  # noisy planes meeting at edges
        m = max(int(np.sqrt(n / 3)), 8)
        sp = int(rng.integers(20, 80))
        u, v = np.meshgrid(np.arange(m) * sp, np.arange(m) * sp, indexing="ij")
        j = int(rng.integers(0, sp // 2 + 1))
        u = u.ravel() + rng.integers(-j, j + 1, m * m)
        v = v.ravel() + rng.integers(-j, j + 1, m * m)
        t = int(rng.integers(0, 60))
        w = rng.integers(-t, t + 1, m * m)
        pts = np.concatenate([np.stack([u, v, w], 1), np.stack([u, w, v + 60], 1), np.stack([w, u + 60, v + 60], 1)])
    elif kind == 1:  # uniform blob
        L = int(50 * n ** (1 / 3) * rng.uniform(0.5, 3))
        pts = rng.integers(0, max(L, 4), (n, 3))
    elif kind == 2:  # lattice with duplicates and exact ties
        g = int(rng.integers(3, 14))
        pts = rng.integers(0, g, (n, 3)) * int(rng.integers(5, 60))
    elif kind == 3:  # curved sheet
        a = rng.uniform(0, 4000, n)
        b = rng.uniform(0, 4000, n)
        pts = np.stack([a, b, 300 * np.sin(a / 500.0) + rng.normal(0, 5, n)], 1)
    else:  # clusters far apart
        c = rng.integers(0, 200000, (int(rng.integers(2, 6)), 3))
        pts = c[rng.integers(0, len(c), n)] + rng.integers(-400, 400, (n, 3))
    pts = np.asarray(pts, dtype=np.int64)
    if rng.random() < 0.7:
        pts = pts[rng.permutation(len(pts))]
    if rng.random() < 0.3:
        pts = pts + rng.integers(-100000, 100000, 3)
    return np.ascontiguousarray(pts.astype(np.int32))


def draw_params(rng, n):
    """The draws of one case after its cloud, in the order main() has always made them; None when n < k (such a
    case draws nothing more)."""
    k = int(rng.integers(2, 33))
    if n < k:
        return None
    radius = float(rng.choice([30.0, 100.0, 100.0, 250.0]))
    max_nn = int(rng.choice([5, 50, 50, 64]))
    return dict(k=k, radius=radius, max_nn=max_nn, th_thickness=int(rng.choice([20, 300, 300, 2000])),
                th_point_count=int(rng.choice([0, 5, 400, 400])), cos_th=float(rng.choice([0.0, 0.5, 0.88, 0.88, 0.99])))


def draw_noise(rng, n):
    """The normal perturbation of one case ([n, 3], or None): the last draws of a case."""
    if rng.random() < 0.5:
        return rng.normal(0, rng.choice([0.05, 0.3]), (n, 3))
    return None


def perturb(normals, noise):
    if noise is None:
        return normals
    nrm = normals + noise
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.ascontiguousarray(nrm)


def replay_case(seed, index):
    """Case `index` of the sequence of `seed`, the way --only reaches it: (xyz, params dict, noise or None)."""
    rng = np.random.default_rng(seed)
    for case in range(index + 1):
        xyz = make_case(rng)
        kw = draw_params(rng, len(xyz))
        if kw is None:
            continue
        noise = draw_noise(rng, len(xyz))
    if kw is None:
        raise ValueError(f"case {index} of seed {seed} is skipped (n < k)")
    return xyz, kw, noise


def draw_limits(lrng, n):
    """A random set of lowered grower limits (api.Context.selftest_grow_limits) for one case.  Drawn from a generator
    of its own, one set per case whether the case runs or not: the cloud stream is shared by every case of a seed, so
    a draw added to it would change all later clouds -- this way a seed gives the same clouds with and without
    --limits.  The pool values are small multiples of n: a cloud whose largest plane needs more ends with
    BS_ERR_NOMEM, which main() accepts only with the pool lowered and only with that message."""
    lim = dict(max_waves=int(lrng.choice([0, 0, 3, 16, 64, 512])),
               pool_cap=int(lrng.choice([0, 0, 12, 24, 48])) * n,
               max_pending=int(lrng.choice([0, 0, 1, 4, 64])),
               pstore_cap=int(lrng.choice([0, 0, 2000, 20000])),
               retry_max_list=int(lrng.choice([-1, -1, 0, 1, 100])),
               retry_big_round=int(lrng.choice([-1, -1, 0, 64])),
               full_refresh=bool(lrng.random() < 0.25))
    return lim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log", default="")
    ap.add_argument("--dump", default="", help="directory for the inputs of failing cases")
    ap.add_argument("--only", type=int, default=-1, help="run just this case of the sequence (the others are only drawn)")
    ap.add_argument("--audit", action="store_true",
                    help="also switch on the replay certificate (bs_set_audit) and count its mismatches as failures")
    ap.add_argument("--repeat", type=int, default=1,
                    help="device runs per case and mode: exposes timing-dependent (nondeterministic) mismatches")
    ap.add_argument("--limits", action="store_true",
                    help="lower a random set of the speculative grower's capacities per case (bs_selftest_grow_limits): "
                         "the recovery paths must give the same bits")
    args = ap.parse_args()
    from buildingsegment_amd import api
    from oracle import oracle as O
    ctx = api.Context(0)
    if args.audit:
        ctx.set_audit(True)
    rng = np.random.default_rng(args.seed)
    lrng = np.random.default_rng([args.seed, 0x6C696D])  # (see draw_limits)
    hit = {}  # --limits: cases in which each recovery path ran
    log = open(args.log, "a") if args.log else sys.stdout
    bad = 0
    t0 = time.time()
    for case in range(args.cases):
        xyz = make_case(rng)
        n = len(xyz)
        lim = draw_limits(lrng, n)
        kw = draw_params(rng, n)
        if kw is None:
            continue
        k, radius, max_nn = kw["k"], kw["radius"], kw["max_nn"]
        p = api.default_params(**kw)
        if args.only >= 0 and case != args.only:  # keep the random stream in step, skip the work
            draw_noise(rng, n)
            continue
        neigh, normals = ctx.knn_normals(xyz, p)
        oneigh, onormals = O.knn_normals(xyz, k=k, radius=radius, max_nn=max_nn)
        ok = np.array_equal(neigh, oneigh) and np.array_equal(normals, onormals)
        nrm = perturb(normals, draw_noise(rng, n))  # perturbed normals: stress the grower with orphans / small planes
        opi, opl = O.region_grow(xyz, nrm, oneigh, th_thickness=p.th_thickness, th_point_count=p.th_point_count,
                                 cos_th=p.cos_th)
        rounds = 0
        why = ""
        for mode in [2] * args.repeat + [1]:
            p.rg_mode = mode
            try:
                if args.limits and mode == 2:
                    ctx.selftest_grow_limits(**lim)
                try:
                    pi, planes = ctx.region_grow(xyz, nrm, oneigh, p)
                except api.BsError as e:
                    # a lowered pool may be too small for the largest plane alone: the specified end of that is
                    # BS_ERR_NOMEM; the case is then run with the full pool and the other limits
                    if not (args.limits and mode == 2 and lim["pool_cap"] and e.status == -3 and "round pool exhausted" in str(e)):
                        raise
                    hit["pool_exhausted"] = hit.get("pool_exhausted", 0) + 1
                    ctx.selftest_grow_limits(**dict(lim, pool_cap=0))
                    pi, planes = ctx.region_grow(xyz, nrm, oneigh, p)
            except api.BsError as e:
                ok = False
                why += f" mode{mode}:{e}"
                continue
            finally:
                ctx.selftest_grow_limits()
            if args.limits and mode == 2:
                gc = ctx.grow_counters()
                for key in ("rounds_capped", "attempts_nomem", "waves_cut", "attempts_stolen", "dropped_pend_count",
                            "dropped_pend_store", "full_refreshes"):
                    hit[key] = hit.get(key, 0) + (gc[key] > 0)
            if mode == 2:
                rounds = ctx.timings()["rg_rounds"]
                tma = ctx.timings()
                if args.audit and (tma["audit_mismatches"] != 0 or tma["audit_attempts"] != tma["n_seed_attempts"]):
                    ok = False
                    why += f" audit:{tma['audit_mismatches']}_mismatches_of_{tma['audit_attempts']}_attempts(finalised:{tma['n_seed_attempts']})"
            okm = np.array_equal(pi, opi) and len(planes) == len(opl["id"])
            if okm and planes:
                okm = (np.array_equal(np.concatenate([q.pointIdx for q in planes]), opl["point_idx"])
                       and np.array_equal(np.stack([q.normal for q in planes]), opl["normal"])
                       and np.array_equal(np.stack([q.center for q in planes]), opl["center"]))
            if not okm:
                why += f" mode{mode}:labels_differ={int((pi != opi).sum())},planes={len(planes)}vs{len(opl['id'])}"
                if planes and len(planes) == len(opl["id"]):  # which plane field differs first
                    for q, (qq, on, oc) in enumerate(zip(planes, opl["normal"], opl["center"])):
                        lst = opl["point_idx"][opl["offset"][q]:opl["offset"][q + 1]]
                        if not (np.array_equal(qq.pointIdx, lst) and np.array_equal(qq.normal, on)
                                and np.array_equal(qq.center, oc)):
                            why += (f",plane{q}(n={len(lst)}):list={np.array_equal(qq.pointIdx, lst)}"
                                    f",normal={list(qq.normal)}vs{list(on)},center={list(qq.center)}vs{list(oc)}")
                            break
            ok = ok and okm
        if not ok and args.dump:
            np.savez_compressed(os.path.join(args.dump, f"fuzz_fail_{args.seed}_{case}.npz"), xyz=xyz, normals=nrm,
                                neigh=oneigh, k=k, th=p.th_thickness, cnt=p.th_point_count, cos=p.cos_th)
        bad += not ok
        print(f"case {case} n={n} k={k} r={radius} M={max_nn} th={p.th_thickness} cnt={p.th_point_count} "
              f"cos={p.cos_th} planes={len(opl['id'])} rounds={rounds} {'ok' if ok else 'MISMATCH' + why}", file=log, flush=True)
    if args.limits:
        print("limits reached (cases): " + " ".join(f"{k}={v}" for k, v in sorted(hit.items())), file=log, flush=True)
    print(f"done: {args.cases} cases, {bad} mismatches, {time.time() - t0:.1f}s", file=log, flush=True)
    ctx.close()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
