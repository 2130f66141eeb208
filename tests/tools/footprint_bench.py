#!/usr/bin/env python3
"""Times bs_footprints_dev per stage (bs_footprint_info, median over repeats after a warm-up) on the rasters of the
urban_50m cloud at bins 100 and 25 mm and on the two long-contour masks of tests/test_gpu_footprints.py, and the
single-threaded restatement (tests/footprint_ref/contour_ref.c) on the same inputs, checking that both agree.
usage: python tests/tools/footprint_bench.py [--reps 7] [--out FILE.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "footprint_ref"))
torch.zeros(1, device="cuda")
from buildingsegment_amd import api, synth  # noqa: E402
import ref  # noqa: E402
from test_gpu_footprints import _comb, _spiral  # noqa: E402

STAGES = ["ms_mask", "ms_close", "ms_label", "ms_trace", "ms_total"]


def run_case(ctx, name, d_img, w, h, reps, iterations):
    for _ in range(2):
        ctx.footprints_dev(d_img.data_ptr(), w, h, iterations=iterations)
    infos, walls = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fp = ctx.footprints_dev(d_img.data_ptr(), w, h, iterations=iterations)
        walls.append((time.perf_counter() - t) * 1e3)
        infos.append(fp.info)
    img = d_img.cpu().numpy()
    t = time.perf_counter()
    r, _ = ref.footprints(img, iterations=iterations)
    ref_ms = (time.perf_counter() - t) * 1e3
    same = (len(r.contours) == len(fp.contours) and all(np.array_equal(a, b) for a, b in zip(fp.contours, r.contours))
            and np.array_equal(fp.area, r.area) and np.array_equal(fp.perimeter, r.perimeter))
    row = {"case": name, "width": w, "height": h, "iterations": iterations, "reps": reps,
           "contours": len(fp.contours), "points": int(sum(len(c) for c in fp.contours)),
           "fg_pixels": fp.info["fg_pixels"], "border_states": fp.info["border_states"],
           "jump_rounds": fp.info["jump_rounds"]}
    for s in STAGES:
        v = [i[s] for i in infos]
        row[s] = round(float(np.median(v)), 3)
        row[s + "_min"] = round(float(np.min(v)), 3)
        row[s + "_max"] = round(float(np.max(v)), 3)
    row["wall_ms_median"] = round(float(np.median(walls)), 3)
    row["restatement_ms"] = round(ref_ms, 1)
    row["equal_to_restatement"] = bool(same)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = api.Context(0)
    rows = []
    xyz = synth.shift_to_origin(synth.urban(50_000_000, seed=4))  # bench.py's urban_50m
    ext = xyz.max(0).astype(np.int32)
    d_xyz = torch.from_numpy(xyz).cuda()
    del xyz
    for bin_ in (100, 25):
        w, h = api.grid_dims(ext, bin_)
        d_img = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        ctx.grid_picture_dev(d_xyz.data_ptr(), d_xyz.shape[0], ext, d_img.data_ptr(), bin=bin_)
        rows.append(run_case(ctx, f"urban_50m_bin{bin_}", d_img, w, h, a.reps, 2))
        del d_img
        torch.cuda.empty_cache()
    del d_xyz
    for name, m in (("spiral_4096", _spiral(4096)), ("comb_1200001x2", _comb(1_200_001))):
        d_img = torch.from_numpy(ref.image_of_mask(m)).cuda()
        rows.append(run_case(ctx, name, d_img, m.shape[1], m.shape[0], a.reps, 0))
        del d_img
    out = {"tool": "tests/tools/footprint_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
