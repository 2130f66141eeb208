#!/usr/bin/env python3
"""Times the roof stage (bs_roofs_dev: vote, fill, figures, heights; HIP events on the context's stream, median of
--reps after 2 warm-ups, with min and max), each stage beside bs_assign_buildings_dev and bs_plane_buildings_dev
re-measured in the same run on the same input:
  - urban at --points (bench.py's urban_50m at the default) at bin 100 and bin 25, labels from bs_segment_dev in the
    same run;
  - the fill alone on a one-pixel ring with one seed at two sizes (R and about 2R rounds), ms_fill beside ms_map of
    bs_building_map_dev on the same image: what a round costs against one pass over the image.
--check compares the device with the restatement tests/roof_ref (the cloud, up to 10 M points) and the rings with
their closed form.
usage: python tests/tools/roof_bench.py [--reps 7] [--points 50000000] [--check] [--out profiles/roofs_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "roof_ref"))
torch.zeros(1, device="cuda")
from buildingsegment_amd import api, synth  # noqa: E402
import roof_ref as rr  # noqa: E402

STREAM = None  # the stream the context runs on
STAGES = ("ms_vote", "ms_fill", "ms_figures", "ms_height")


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


def same(r, want, roof, support, height):
    return bool(np.array_equal(roof, want.roof) and np.array_equal(support, want.support) and
                np.array_equal(height, want.height) and all(np.array_equal(getattr(r, k), getattr(want, k)) for k in rr.FIGURES) and
                all(getattr(r, k) == getattr(want, k) for k in rr.TOTALS))


def cloud_case(ctx, xyz, d_xyz, d_plane, planes, ext, bin_, reps, check):
    n, n_planes = len(xyz), len(planes)
    normal = np.array([p.normal for p in planes], np.float64).reshape(n_planes, 3)
    center = np.array([p.center for p in planes], np.int32).reshape(n_planes, 3)
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

    _, asg, asg_kernel = timed(assign, reps)
    votes, vot, _ = timed(lambda: ctx.plane_buildings_dev(d_plane.data_ptr(), d_bidx.data_ptr(), n, n_planes, b.n_buildings), reps)
    home = api.roof_homes(normal, votes.plane_building, votes.votes_in, votes.votes_total)
    d_roof, d_sup, d_hgt = (torch.empty((h, w), dtype=torch.int32, device="cuda") for _ in range(3))
    r, whole, runs = timed(lambda: ctx.roofs_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), w, h, d_plane.data_ptr(), home, normal,
                                                 center, d_roof.data_ptr(), d_sup.data_ptr(), d_hgt.data_ptr(), bin=bin_,
                                                 ground_th=th), reps)
    row = {"case": f"urban_{n}_bin{bin_}", "points": n, "bin": bin_, "width": w, "height": h, "reps": reps, "ground_th": th,
           "planes": n_planes, "buildings": b.n_buildings, "planes_with_a_home": int((home >= 0).sum()),
           "seeded_pixels": r.seeded_pixels, "filled_pixels": r.filled_pixels, "unroofed_pixels": r.unroofed_pixels,
           "fill_rounds": r.fill_rounds, "supporting_points": int(r.n_support.sum()),
           "roofs_dev_ms": stat(whole), "assign_buildings_dev_ms": stat(asg), "assign_kernel_ms": stat(asg_kernel),
           "plane_buildings_dev_ms": stat(vot), "ms_map": round(b.info["ms_map"], 3)}
    for k in STAGES:
        row[k] = stat([x.info[k] for x in runs])
        row[f"ratio_{k[3:]}_over_assign_kernel"] = round(row[k]["median"] / row["assign_kernel_ms"]["median"], 3)
        row[f"ratio_{k[3:]}_over_plane_buildings"] = round(row[k]["median"] / row["plane_buildings_dev_ms"]["median"], 3)
    row["ms_stages_sum"] = round(sum(row[k]["median"] for k in STAGES), 3)
    row["dominant_stage"] = max(STAGES, key=lambda k: row[k]["median"])
    if check and n <= 10_000_000:
        want = rr.roofs(xyz, d_map.cpu().numpy(), d_plane.cpu().numpy(), n_planes, home, normal, center, bin_, th, 1)
        row["equal_to_restatement"] = same(r, want, d_roof.cpu().numpy(), d_sup.cpu().numpy(), d_hgt.cpu().numpy())
    print(json.dumps(row), flush=True)
    return row


def ring_case(ctx, size, reps, check):
    """a one-pixel ring along the border of a size x size image, one seed: 2 * size - 2 rounds"""
    bmap = np.full((size, size), -1, np.int32)
    bmap[0, :] = bmap[-1, :] = bmap[:, 0] = bmap[:, -1] = 0
    xyz = np.array([[5, 5, 100]], np.int32)
    plane, home = np.ones(1, np.int32), np.zeros(1, np.int32)
    normal, center = np.array([[0.0, 0.0, 1.0]]), np.array([[0, 0, 100]], np.int32)
    d_xyz, d_plane, d_map = torch.from_numpy(xyz).cuda(), torch.from_numpy(plane).cuda(), torch.from_numpy(bmap).cuda()
    # one pass over an image of this size: the map kernel of bs_building_map_dev (which would give the ring's inside
    # to the ring: the roof stage gets the hand-made map)
    d_mask, d_tmp = (d_map >= 0).to(torch.uint8), torch.empty_like(d_map)
    _, _, maps = timed(lambda: ctx.building_map_dev(d_mask.data_ptr(), size, size, d_tmp.data_ptr()).info["ms_map"], reps)
    d_roof, d_sup, d_hgt = (torch.empty((size, size), dtype=torch.int32, device="cuda") for _ in range(3))
    r, _, runs = timed(lambda: ctx.roofs_dev(d_xyz.data_ptr(), 1, d_map.data_ptr(), size, size, d_plane.data_ptr(), home, normal,
                                             center, d_roof.data_ptr(), d_sup.data_ptr(), d_hgt.data_ptr(), bin=10), reps)
    row = {"case": f"ring_{size}", "width": size, "height": size, "reps": reps, "fill_rounds": r.fill_rounds,
           "filled_pixels": r.filled_pixels, "ms_fill": stat([x.info["ms_fill"] for x in runs]), "ms_map": stat(maps)}
    row["us_per_round"] = round(1000.0 * row["ms_fill"]["median"] / r.fill_rounds, 3)
    row["rounds_per_image_pass"] = round(row["ms_map"]["median"] * r.fill_rounds / row["ms_fill"]["median"], 3)
    if check:
        # (thousands of whole-image rounds are beyond the restatement: the result is known in closed form)
        roof, hgt = d_roof.cpu().numpy(), d_hgt.cpu().numpy()
        row["equal_to_closed_form"] = bool(np.array_equal(roof, np.where(bmap == 0, 1, -1)) and r.fill_rounds == 2 * size - 2 and
                                           np.array_equal(hgt, np.where(bmap == 0, 100, rr.I32_MIN)) and
                                           r.filled_pixels == 4 * size - 5 and int(d_sup.sum().item()) == 1)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--ring", type=int, default=1024)
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
    d_plane = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.segment_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), api.default_params(k=15))
    planes = ctx.planes_fetch()
    for bin_ in (100, 25):
        rows.append(cloud_case(ctx, xyz, d_xyz, d_plane, planes, ext, bin_, a.reps, a.check))
        torch.cuda.empty_cache()
    del d_xyz, d_plane, xyz, planes
    rings = [ring_case(ctx, s, a.reps, a.check) for s in (a.ring, 2 * a.ring)]
    rows += rings
    rows.append({"case": "ring_rounds_doubled", "fill_rounds_ratio": round(rings[1]["fill_rounds"] / rings[0]["fill_rounds"], 3),
                 "ms_fill_ratio": round(rings[1]["ms_fill"]["median"] / rings[0]["ms_fill"]["median"], 3)})
    out = {"tool": "tests/tools/roof_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
