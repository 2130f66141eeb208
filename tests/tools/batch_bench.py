#!/usr/bin/env python3
"""Times one bs_segment_batch_dev call against the loop of per-tile bs_segment_dev calls over the same tiles (HIP
events on the context's stream; median, min and max of --reps runs after 2 warm-ups) for three cases: 32 facade 1 M
tiles, 256 uniform 200 k tiles, and the urban 50 M cloud as a batch of one.  Also checks that both give the same rows,
normals and labels.
usage: python tests/tools/batch_bench.py [--reps 7] [--cases facade_32x1m,uniform_256x200k,urban_50m_x1] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
torch.zeros(1, device="cuda")
from buildingsegment_amd import api, synth  # noqa: E402

CASES = {
    "facade_32x1m": lambda: [synth.facade(n_side=1000, seed=2 + s) for s in range(32)],
    "uniform_256x200k": lambda: [synth.uniform(200_000, seed=10 + s) for s in range(256)],
    "urban_50m_x1": lambda: [synth.urban(50_000_000, seed=4)],  # (bench.py's urban_50m cloud)
}


def timed(fn, reps, warm=2):
    st = torch.cuda.current_stream()
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3),
            "max_ms": round(float(np.max(ms)), 3)}


def run_case(ctx, name, reps):
    t0 = time.perf_counter()
    tiles = CASES[name]()
    gen_s = time.perf_counter() - t0
    p = api.default_params(k=16)
    xyz, off = api.pack_tiles(tiles)
    del tiles
    n, nt = len(xyz), len(off) - 1
    d_xyz = torch.from_numpy(xyz).cuda()
    del xyz
    outs = []
    for _ in range(2):
        outs.append((torch.empty((n, p.k), dtype=torch.int32, device="cuda"),
                     torch.empty((n, 3), dtype=torch.float64, device="cuda"),
                     torch.empty(n, dtype=torch.int32, device="cuda")))
    (bn, br, bp), (ln, lr, lp) = outs

    def batch():
        ctx.segment_batch_dev(d_xyz.data_ptr(), off, bp.data_ptr(), p, bn.data_ptr(), br.data_ptr())

    def loop():
        for t in range(nt):
            s = slice(int(off[t]), int(off[t + 1]))
            ctx.segment_dev(d_xyz[s].data_ptr(), s.stop - s.start, lp[s].data_ptr(), p, ln[s].data_ptr(),
                            lr[s].data_ptr())

    mb = timed(batch, reps)
    tb = ctx.timings()
    ml = timed(loop, reps)
    # the loop leaves rows in tile-local numbering as well: the two must agree
    equal = bool(torch.equal(bn, ln) and torch.equal(br, lr) and torch.equal(bp, lp))
    row = {"case": name, "n_tiles": nt, "n_points": n, "k": p.k, "reps": reps, "warmups": 2,
           "batch": stats(mb), "loop": stats(ml), "speedup_median": round(float(np.median(ml) / np.median(mb)), 3),
           "batch_stages_last_ms": {"grid": round(tb["grid_ms"], 3), "knn": round(tb["knn_ms"], 3),
                                    "grow": round(tb["grow_ms"], 3)},
           "batch_mpoints_per_s": round(n / np.median(mb) / 1e3, 1), "equal": equal,
           "generate_s": round(gen_s, 1)}
    print(json.dumps(row), flush=True)
    del d_xyz, outs, bn, br, bp, ln, lr, lp
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.json"))
    a = ap.parse_args()
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)  # the events below time the context's own work
    rows = [run_case(ctx, c, a.reps) for c in a.cases.split(",")]
    ctx.close()
    doc = {"tool": "tests/tools/batch_bench.py", "device": torch.cuda.get_device_name(0),
           "timing": "HIP events around each call on the context's stream, after 2 warm-ups", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    ok = all(r["equal"] for r in rows)
    print("batch_bench:", "outputs equal" if ok else "OUTPUTS DIFFER")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
