#!/usr/bin/env python3
"""Times the facet outlines (bs_facet_outlines_count_dev: half-edges, leaders, rank, rings; bs_facet_outlines_emit_dev) on
urban at --points (bench.py's urban_50m at the default) at bin 100 and bin 25, from bs_segment_dev -> buildings -> roofs
-> solids -> facets in the same run.  HIP events on the context's stream, median of --reps after 2 warm-ups, with min and
max.  Beside them, re-measured in the same run on the same image: bs_roof_facets_dev, and device-to-device copies of as
many bytes as the stage must touch (label and top read once: 20 per pixel; per half-edge what the 2 R jump rounds move: 24
each).
--check compares every array with the restatement tests/outline_ref (the cloud capped at 5 M points).
usage: python tests/tools/outline_bench.py [--reps 7] [--points 50000000] [--check] [--out profiles/facet_outlines_bench.json]"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
torch.zeros(1, device="cuda")
from buildingsegment_amd import api, synth  # noqa: E402

STREAM = None  # the stream the context runs on
STAGES = ("ms_halfedges", "ms_leaders", "ms_rank", "ms_rings")


def outline_ref():
    spec = importlib.util.spec_from_file_location("outline_ref", os.path.join(ROOT, "tests", "outline_ref", "outline_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["outline_ref"] = mod
    spec.loader.exec_module(mod)
    return mod


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


def copy_ms(nbytes, reps):
    """a device-to-device copy of nbytes on the context's stream"""
    n = max(nbytes // 4, 1)
    src, dst = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def fn():
        with torch.cuda.stream(STREAM):
            dst.copy_(src)

    return timed(fn, reps)[1]


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
    ctx.assign_buildings_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), b, d_bidx.data_ptr(), bin=bin_, ground_th=th)
    votes = ctx.plane_buildings_dev(d_plane.data_ptr(), d_bidx.data_ptr(), n, n_planes, b.n_buildings)
    home = api.roof_homes(normal, votes.plane_building, votes.votes_in, votes.votes_total)
    d_roof, d_hgt = (torch.empty((h, w), dtype=torch.int32, device="cuda") for _ in range(2))
    r = ctx.roofs_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), w, h, d_plane.data_ptr(), home, normal, center, d_roof.data_ptr(), 0,
                      d_hgt.data_ptr(), bin=bin_, ground_th=th)
    del d_bidx, d_hgt, d_mask
    base_z, flat = api._solid_defaults(b, None, None)
    d_top = torch.empty((h, w, 4), dtype=torch.int32, device="cuda")
    ctx.solids_dev(d_map.data_ptr(), d_roof.data_ptr(), w, h, normal, center, r.z_min, r.z_max, bin_, base_z, flat,
                   d_top=d_top.data_ptr())
    d_facet = torch.empty((h, w), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    f, facets_ms, _ = timed(lambda: ctx.roof_facets_dev(d_map.data_ptr(), d_roof.data_ptr(), d_top.data_ptr(), w, h,
                                                        b.n_buildings, n_planes, d_facet.data_ptr()), reps)
    count = lambda: ctx.facet_outlines_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h, f.n_facets)  # noqa: E731
    o, whole, runs = timed(count, reps)
    d_xy = torch.empty((o.n_vertices, 2), dtype=torch.int32, device="cuda")
    d_z = torch.empty((o.n_vertices,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _, emit_ms, _ = timed(lambda: ctx.facet_outlines_emit_dev(d_xy.data_ptr(), d_z.data_ptr()), reps)
    npix = w * h
    rounds = max(int(o.n_half) - 1, 1).bit_length()
    bytes_image, bytes_jumps = 20 * npix, 24 * 2 * rounds * o.n_half
    row = {"case": f"urban_{n}_bin{bin_}", "points": n, "bin": bin_, "width": w, "height": h, "reps": reps,
           "buildings": b.n_buildings, "facets": f.n_facets, "n_half": o.n_half, "n_rings": o.n_rings,
           "n_vertices": o.n_vertices, "holes": int((o.ring_area2 < 0).sum()), "longest_ring": int(o.ring_length.max()),
           "jump_rounds": 2 * rounds, "bytes_image": bytes_image, "bytes_jumps": bytes_jumps,
           "facet_outlines_count_dev_ms": stat(whole), "facet_outlines_emit_dev_ms": stat(emit_ms),
           "roof_facets_dev_ms": stat(facets_ms), "copy_image_ms": stat(copy_ms(bytes_image, reps)),
           "copy_jumps_ms": stat(copy_ms(bytes_jumps, reps))}
    for k in STAGES:
        row[k] = stat([x.info[k] for x in runs])
    row["ms_stages_sum"] = round(sum(row[k]["median"] for k in STAGES), 3)
    row["dominant_stage"] = max(STAGES, key=lambda k: row[k]["median"])
    row["count_over_roof_facets"] = round(row["facet_outlines_count_dev_ms"]["median"] / row["roof_facets_dev_ms"]["median"], 3)
    row["copy_over_stages"] = round((row["copy_image_ms"]["median"] + row["copy_jumps_ms"]["median"]) / row["ms_stages_sum"], 3)
    if check:
        orf = outline_ref()
        o.xy, o.z = d_xy.cpu().numpy(), d_z.cpu().numpy()
        facet = d_facet.cpu().numpy()
        want = orf.outlines(facet, d_top.cpu().numpy(), f.n_facets)
        diff = orf.same(o, want)
        row["equal_to_restatement"] = diff is None
        if diff is not None:
            row["first_difference"] = diff
        per = np.zeros(f.n_facets, np.int64)
        np.add.at(per, o.ring_label, o.ring_length)
        row["lengths_equal_facet_edges"] = bool(np.array_equal(per, f.facet_inner_edges + f.facet_outer_edges))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out_path = a.out or os.path.join(ROOT, "profiles", "facet_outlines_bench_check.json" if a.check else "facet_outlines_bench.json")
    global STREAM
    ctx = api.Context(0)
    STREAM = torch.cuda.Stream()
    ctx.set_stream(STREAM.cuda_stream)
    n = min(a.points, 5_000_000) if a.check else a.points
    xyz = synth.shift_to_origin(synth.urban(n, seed=4))  # bench.py's urban_50m at the default size
    n = len(xyz)
    ext = xyz.max(0).astype(np.int32)
    d_xyz = torch.from_numpy(xyz).cuda()
    d_plane = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.segment_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), api.default_params(k=15))
    planes = ctx.planes_fetch()
    rows = []
    for bin_ in (100, 25):
        rows.append(cloud_case(ctx, xyz, d_xyz, d_plane, planes, ext, bin_, a.reps, a.check))
        torch.cuda.empty_cache()
    out = {"tool": "tests/tools/outline_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
