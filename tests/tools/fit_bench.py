#!/usr/bin/env python3
"""Times the plane fit (bs_plane_fit_dev: sums, moments, solve, residuals; HIP events on the context's stream, median
of --reps after 2 warm-ups, with min and max) on urban at --points (bench.py's urban_50m at the default) with the labels
of bs_segment_dev from the same run, beside the bs_assign_buildings_dev kernel and bs_plane_buildings_dev re-measured
in the same run on the same points.  Two orders of the same points: as the cloud comes (shuffled: every lane of a wave
carries another plane) and sorted by label (whole waves of one plane).  The alternative to reducing by label in LDS --
sorting the point indices by label first -- is bounded from below by the radix sort alone (torch.sort of the labels:
keys and indices), timed in the same run.
--check compares every array with the restatement tests/fit_ref on urban at 5 M points.
usage: python tests/tools/fit_bench.py [--reps 7] [--points 50000000] [--check] [--out profiles/plane_fit_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "fit_ref"))
torch.zeros(1, device="cuda")
from buildingsegment_amd import api, synth  # noqa: E402
import fit_ref as fr  # noqa: E402

STREAM = None  # the stream the context runs on
STAGES = ("ms_sums", "ms_moments", "ms_solve", "ms_residuals")


def stat(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def timed(fn, reps):
    """torch events on the context's stream around fn(), after 2 warm-ups; returns (last result, ms, all results)"""
    outs, ms = [], []
    for it in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(STREAM)
        out = fn()
        b.record(STREAM)
        b.synchronize()
        if it >= 2:
            ms.append(a.elapsed_time(b))
            outs.append(out)
    return out, ms, outs


def segment(ctx, points):
    xyz = synth.shift_to_origin(synth.urban(points, seed=4))  # bench.py's urban_50m at the default size
    d_xyz = torch.from_numpy(xyz).cuda()
    d_plane = torch.empty(len(xyz), dtype=torch.int32, device="cuda")
    ctx.segment_dev(d_xyz.data_ptr(), len(xyz), d_plane.data_ptr(), api.default_params(k=15))
    return xyz, d_xyz, d_plane, len(ctx.planes_fetch())


def fit_row(ctx, name, d_xyz, d_plane, n_planes, reps, yard):
    n = len(d_plane)
    d_res = torch.empty(n, dtype=torch.int32, device="cuda")
    f, whole, runs = timed(lambda: ctx.plane_fit_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), n_planes, d_res.data_ptr()), reps)
    _, bare, _ = timed(lambda: ctx.plane_fit_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), n_planes), reps)
    row = {"case": name, "points": n, "planes": n_planes, "reps": reps, "labelled_points": int(f.n_points.sum()),
           "fitted": int((f.status == 0).sum()), "too_few": int((f.status == 1).sum()), "too_large": int((f.status == 2).sum()),
           "planes_above_the_lds_tables": max(n_planes - 3072, 0), "r_abs_max": int(f.r_abs_max.max(initial=0)),
           "plane_fit_dev_ms": stat(whole), "plane_fit_dev_without_residual_image_ms": stat(bare)}
    for k in STAGES:
        row[k] = stat([x.info[k] for x in runs])
        for y, v in yard.items():
            row[f"ratio_{k[3:]}_over_{y}"] = round(row[k]["median"] / v, 3)
    row["ms_stages_sum"] = round(sum(row[k]["median"] for k in STAGES), 3)
    print(json.dumps(row), flush=True)
    return row, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    global STREAM
    ctx = api.Context(0)
    STREAM = torch.cuda.Stream()
    ctx.set_stream(STREAM.cuda_stream)
    rows = []
    xyz, d_xyz, d_plane, n_planes = segment(ctx, a.points)
    n, ext, bin_ = len(xyz), xyz.max(0).astype(np.int32), 100
    del xyz
    # the yardsticks: the assignment kernel (16 bytes per point, as every pass of the fit) and the plane votes
    w, h = api.grid_dims(ext, bin_)
    d_img = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    th = ctx.grid_picture_dev(d_xyz.data_ptr(), n, ext, d_img.data_ptr(), bin=bin_)
    d_mask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    ctx.footprints_dev(d_img.data_ptr(), w, h, d_mask=d_mask.data_ptr())
    del d_img
    d_map = torch.empty((h, w), dtype=torch.int32, device="cuda")
    b = ctx.building_map_dev(d_mask.data_ptr(), w, h, d_map.data_ptr())
    d_bidx = torch.empty(n, dtype=torch.int32, device="cuda")

    def assign():
        ctx.assign_buildings_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), b, d_bidx.data_ptr(), bin=bin_, ground_th=th)
        return b.info["ms_assign"]

    _, _, asg_kernel = timed(assign, a.reps)
    _, vot, _ = timed(lambda: ctx.plane_buildings_dev(d_plane.data_ptr(), d_bidx.data_ptr(), n, n_planes, b.n_buildings), a.reps)
    yard = {"assign_kernel": float(np.median(asg_kernel)), "plane_buildings": float(np.median(vot))}
    rows.append({"case": "yardsticks", "points": n, "assign_kernel_ms": stat(asg_kernel), "plane_buildings_dev_ms": stat(vot)})
    print(json.dumps(rows[-1]), flush=True)
    del d_bidx, d_map, d_mask
    torch.cuda.empty_cache()

    row, f0 = fit_row(ctx, f"urban_{n}_as_it_comes", d_xyz, d_plane, n_planes, a.reps, yard)
    rows.append(row)
    # the lower bound of the other candidate: a radix sort of the labels with the point indices
    with torch.cuda.stream(STREAM):
        _, srt, _ = timed(lambda: torch.sort(d_plane), a.reps)
        order = torch.sort(d_plane).indices
        s_xyz, s_plane = d_xyz[order].contiguous(), d_plane[order].contiguous()
        del order
    STREAM.synchronize()
    rows.append({"case": "sort_labels_with_indices", "points": n, "torch_sort_ms": stat(srt),
                 "ratio_over_fit_stages_sum": round(float(np.median(srt)) / row["ms_stages_sum"], 3)})
    print(json.dumps(rows[-1]), flush=True)
    del d_xyz, d_plane
    torch.cuda.empty_cache()
    row, f1 = fit_row(ctx, f"urban_{n}_sorted_by_label", s_xyz, s_plane, n_planes, a.reps, yard)
    row["equal_to_the_other_order"] = bool(all(np.array_equal(getattr(f0, k), getattr(f1, k)) for k in fr.ARRAYS))
    rows.append(row)
    del s_xyz, s_plane
    torch.cuda.empty_cache()

    if a.check:
        xyz, d_xyz, d_plane, m = segment(ctx, min(a.points, 5_000_000))
        d_res = torch.empty(len(xyz), dtype=torch.int32, device="cuda")
        f = ctx.plane_fit_dev(d_xyz.data_ptr(), len(xyz), d_plane.data_ptr(), m, d_res.data_ptr())
        want = fr.plane_fit(xyz, d_plane.cpu().numpy(), m)
        eq = {k: bool(np.array_equal(getattr(f, k).view(np.int64) if k == "normal" else getattr(f, k),
                                     getattr(want, k).view(np.int64) if k == "normal" else getattr(want, k))) for k in fr.ARRAYS}
        eq["residual"] = bool(np.array_equal(d_res.cpu().numpy(), want.residual))
        rows.append({"case": f"check_urban_{len(xyz)}", "planes": m, "fitted": int((f.status == 0).sum()),
                     "equal_to_restatement": all(eq.values()), "arrays": eq})
        print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tests/tools/fit_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
