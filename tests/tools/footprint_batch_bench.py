#!/usr/bin/env python3
"""Times one bs_grid_picture_batch_dev call against the loop of per-tile bs_grid_picture_dev calls, and one
bs_footprints_batch_dev call against the loop of per-tile bs_footprints_dev calls, over the same tiles (HIP events on
the context's stream; median, min and max of --reps runs after 2 warm-ups).  Cases: 256 urban tiles of 200 k points,
2 000 urban tiles of about 5 k points, and the urban 50 M cloud as a batch of one.  Also checks that both forms give
the same images, thresholds and contours.
usage: python tests/tools/footprint_batch_bench.py [--reps 7] [--cases urban_256x200k,urban_2000x5k,urban_50m_x1]
       [--out FILE]"""
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


def pieces(n_tiles, per, seed, cell=20_000):
    """n_tiles spatially compact tiles of `per` points: one urban cloud in (x, y) cell order, cut into equal runs."""
    xyz = synth.urban(n_tiles * per, seed=seed)
    key = (xyz[:, 0] // cell).astype(np.int64) * (1 << 20) + xyz[:, 1] // cell
    xyz = xyz[np.argsort(key, kind="stable")]
    return [xyz[t * per:(t + 1) * per] for t in range(n_tiles)]


CASES = {
    "urban_256x200k": lambda: [synth.urban(200_000, seed=10 + s) for s in range(256)],
    "urban_2000x5k": lambda: pieces(2000, 5_000, seed=1000),
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


def same_contours(a, b):
    return (len(a.contours) == len(b.contours) and all(np.array_equal(x, y) for x, y in zip(a.contours, b.contours))
            and np.array_equal(a.area, b.area) and np.array_equal(a.perimeter, b.perimeter))


def run_case(ctx, name, reps):
    t0 = time.perf_counter()
    tiles = CASES[name]()
    gen_s = time.perf_counter() - t0
    xyz, off = api.pack_tiles(tiles)
    del tiles
    n, nt = len(xyz), len(off) - 1
    d_xyz = torch.from_numpy(xyz).cuda()
    del xyz
    ctx.shift_tiles_to_origin_dev(d_xyz.data_ptr(), off)
    box = ctx.tile_boxes_dev(d_xyz.data_ptr(), off)
    ext = box[:, 3:] - box[:, :3]
    w, h, po = api.grid_dims_batch(ext)
    npix = int(po[-1])
    bimg = torch.empty(3 * npix, dtype=torch.float64, device="cuda")
    limg = torch.empty(3 * npix, dtype=torch.float64, device="cuda")
    res = {}

    def r_batch():
        res["bth"] = ctx.grid_picture_batch_dev(d_xyz.data_ptr(), off, ext, bimg.data_ptr())

    def r_loop():
        res["lth"] = [ctx.grid_picture_dev(d_xyz[int(off[t]):int(off[t + 1])].data_ptr(), int(off[t + 1] - off[t]),
                                           ext[t], limg[3 * int(po[t]):].data_ptr()) for t in range(nt)]

    def f_batch():
        res["bfp"] = ctx.footprints_batch_dev(bimg.data_ptr(), w, h)

    def f_loop():
        res["lfp"] = [ctx.footprints_dev(limg[3 * int(po[t]):].data_ptr(), int(w[t]), int(h[t])) for t in range(nt)]

    rb, rl = timed(r_batch, reps), timed(r_loop, reps)
    fb, fl = timed(f_batch, reps), timed(f_loop, reps)
    eq_raster = bool(torch.equal(bimg, limg)) and list(res["bth"]) == res["lth"]
    eq_fp = all(same_contours(a, b) for a, b in zip(res["bfp"], res["lfp"]))
    inf = res["bfp"][0].info
    row = {"case": name, "n_tiles": nt, "n_points": n, "pixels": npix, "contours": int(inf["components"]),
           "reps": reps, "warmups": 2,
           "raster": {"batch": stats(rb), "loop": stats(rl), "speedup_median": round(float(np.median(rl) / np.median(rb)), 3),
                      "equal": eq_raster},
           "footprints": {"batch": stats(fb), "loop": stats(fl),
                          "speedup_median": round(float(np.median(fl) / np.median(fb)), 3), "equal": eq_fp,
                          "batch_stages_last_ms": {k: round(inf[k], 3) for k in ("ms_mask", "ms_close", "ms_label",
                                                                                 "ms_trace")}},
           "generate_s": round(gen_s, 1)}
    print(json.dumps(row), flush=True)
    del d_xyz, bimg, limg, res
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "footprints_batch_bench.json"))
    a = ap.parse_args()
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)  # the events below time the context's own work
    rows = [run_case(ctx, c, a.reps) for c in a.cases.split(",")]
    ctx.close()
    doc = {"tool": "tests/tools/footprint_batch_bench.py", "device": torch.cuda.get_device_name(0),
           "timing": "HIP events around each call (host round trips included) on the context's stream, after 2 "
                     "warm-ups", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    ok = all(r["raster"]["equal"] and r["footprints"]["equal"] for r in rows)
    print("footprint_batch_bench:", "outputs equal" if ok else "OUTPUTS DIFFER")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
