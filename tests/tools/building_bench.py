#!/usr/bin/env python3
"""Times the building map, the point assignment and the plane votes, each beside an existing, unchanged code path on
the same input (median of --reps after 2 warm-ups, with min and max; HIP events on the context's stream):
  - labelling pass 1 of bs_building_map_dev (tile + seam + flatten kernels, bs_buildings.ms_label_mask) beside
    bs_footprint_info.ms_label of bs_footprints_dev (init + union + flatten kernels AND the flag pass, three scans and
    a small read-back) on the same closed mask; ms_label_mask + ms_number (the new path's flag + scan + read-back) is
    the same span as ms_label, with one scan where the tracer needs three;
  - bs_assign_buildings_dev beside bs_grid_picture_dev on the same 50 M points (torch events around the whole call
    on the context's stream: both calls synchronise at their end);
  - the votes and the whole chain (map + assignment + votes) on their own.
Every device result is compared with the restatement tests/building_ref where that is affordable (--check).
usage: python tests/tools/building_bench.py [--reps 7] [--points 50000000] [--check] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "footprint_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "building_ref"))
torch.zeros(1, device="cuda")
from buildingsegment_amd import api, synth  # noqa: E402
import building_ref as bref  # noqa: E402
import ref  # noqa: E402
from test_gpu_footprints import _spiral  # noqa: E402


def stat(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


STREAM = None  # the stream the context runs on


def timed(fn, reps):
    """torch events on the context's stream around fn(), after 2 warm-ups"""
    out = None
    for _ in range(2):
        out = fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(STREAM)
        out = fn()
        b.record(STREAM)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, ms


def label_case(ctx, name, d_img, w, h, iterations, reps, check):
    d_mask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    d_map = torch.empty((h, w), dtype=torch.int32, device="cuda")
    old, new = [], []
    for it in range(reps + 2):
        fp = ctx.footprints_dev(d_img.data_ptr(), w, h, iterations=iterations, d_mask=d_mask.data_ptr())
        b = ctx.building_map_dev(d_mask.data_ptr(), w, h, d_map.data_ptr())
        if it >= 2:
            old.append(fp.info["ms_label"])
            new.append(b.info)
    row = {"case": name, "width": w, "height": h, "iterations": iterations, "reps": reps, "contours": len(fp.contours),
           "buildings": b.n_buildings, "footprints_ms_label": stat(old)}
    for k in ("ms_label_mask", "ms_label_fill", "ms_number", "ms_map"):
        row[k] = stat([i[k] for i in new])
    row["ms_label_mask_plus_number"] = stat([i["ms_label_mask"] + i["ms_number"] for i in new])
    row["ms_building_map_total"] = stat([i["ms_label_mask"] + i["ms_label_fill"] + i["ms_number"] + i["ms_map"] for i in new])
    row["ratio_new_over_old_kernels_only"] = round(row["ms_label_mask"]["median"] / row["footprints_ms_label"]["median"], 4)
    row["ratio_new_over_old_same_span"] = round(row["ms_label_mask_plus_number"]["median"] /
                                                row["footprints_ms_label"]["median"], 4)
    same = b.n_buildings == len(fp.contours) and all(tuple(c[0]) == tuple(s) for c, s in zip(fp.contours, b.start_xy))
    row["building_c_is_contour_c"] = bool(same)
    if check:
        r = bref.building_map(d_mask.cpu().numpy())
        row["equal_to_restatement"] = bool(np.array_equal(d_map.cpu().numpy(), r.map) and
                                           all(np.array_equal(getattr(b, k), getattr(r, k))
                                               for k in ("start_xy", "bbox", "pixels", "fg_pixels")))
    print(json.dumps(row), flush=True)
    return row, b, d_mask, d_map


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
    xyz = synth.shift_to_origin(synth.urban(a.points, seed=4))  # bench.py's urban_50m at the default size
    n = len(xyz)
    ext = xyz.max(0).astype(np.int32)
    d_xyz = torch.from_numpy(xyz).cuda()
    p = api.default_params(k=15)
    d_plane = torch.empty(n, dtype=torch.int32, device="cuda")
    _, seg_ms = timed(lambda: ctx.segment_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), p), 1)
    n_planes = len(ctx.planes_fetch())
    for bin_ in (100, 25):
        w, h = api.grid_dims(ext, bin_)
        d_img = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        th, ras = timed(lambda: ctx.grid_picture_dev(d_xyz.data_ptr(), n, ext, d_img.data_ptr(), bin=bin_), a.reps)
        row, b, d_mask, d_map = label_case(ctx, f"urban_{n}_bin{bin_}", d_img, w, h, 2, a.reps, a.check)
        del d_img
        d_bidx = torch.empty(n, dtype=torch.int32, device="cuda")
        asg_kernel = []

        def assign():
            ctx.assign_buildings_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), b, d_bidx.data_ptr(), bin=bin_, ground_th=th)
            asg_kernel.append(b.info["ms_assign"])

        _, asg = timed(assign, a.reps)
        votes, vot = timed(lambda: ctx.plane_buildings_dev(d_plane.data_ptr(), d_bidx.data_ptr(), n, n_planes,
                                                           b.n_buildings), a.reps)

        def chain():
            bb = ctx.building_map_dev(d_mask.data_ptr(), w, h, d_map.data_ptr())
            ctx.assign_buildings_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), bb, d_bidx.data_ptr(), bin=bin_, ground_th=th)
            return ctx.plane_buildings_dev(d_plane.data_ptr(), d_bidx.data_ptr(), n, n_planes, bb.n_buildings)

        _, cha = timed(chain, a.reps)
        row.update({"points": n, "ground_th": th, "planes": n_planes, "grid_picture_dev_ms": stat(ras),
                    "assign_buildings_dev_ms": stat(asg), "assign_kernel_ms": stat(asg_kernel[2:]),
                    "ratio_assign_over_grid_picture": round(float(np.median(asg) / np.median(ras)), 4),
                    "plane_buildings_dev_ms": stat(vot), "chain_map_assign_votes_ms": stat(cha),
                    "segment_dev_ms": round(float(seg_ms[0]), 1),
                    "points_in_a_building": int((d_bidx >= 0).sum().item()),
                    "planes_with_a_building": int((votes.plane_building >= 0).sum())})
        if a.check:
            host = bref.assign(xyz, d_map.cpu().numpy(), b.n_buildings, bin_, th)
            row["assignment_equal_to_restatement"] = bool(
                np.array_equal(d_bidx.cpu().numpy(), host.building_idx) and
                all(np.array_equal(getattr(b, k), getattr(host, k)) for k in ("n_points", "n_above", "z_min", "z_max", "z_sum")))
            want = bref.votes(d_plane.cpu().numpy(), host.building_idx, n_planes, b.n_buildings)
            row["votes_equal_to_restatement"] = bool(all(np.array_equal(x, y) for x, y in zip(
                (votes.plane_building, votes.votes_in, votes.votes_total, votes.votes_outside), want)))
            row["above_ground_unassigned"] = int(((host.building_idx < 0) & host.above).sum())
        print(json.dumps(row), flush=True)
        rows.append(row)
        del d_mask, d_map, d_bidx
        torch.cuda.empty_cache()
    del d_xyz, d_plane, xyz
    m = _spiral(4096)
    d_img = torch.from_numpy(ref.image_of_mask(m)).cuda()
    rows.append(label_case(ctx, "spiral_4096", d_img, 4096, 4096, 0, a.reps, a.check)[0])
    out = {"tool": "tests/tools/building_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
