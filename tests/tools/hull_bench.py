#!/usr/bin/env python3
"""Times the oriented boxes (bs_label_hulls_count_dev: outlines, candidates, rounds, order, boxes; bs_label_hulls_emit_dev) on
urban at --points (bench.py's urban_50m at the default) at bin 100, on the building map and on the facet image, from
bs_segment_dev -> buildings -> roofs -> solids -> facets in the same run.  HIP events on the context's stream, median of
--reps after 2 warm-ups, with min and max.  Beside them, re-measured in the same run on the same image:
bs_facet_outlines_count_dev without top (the stage runs it first: the yardstick), and a device-to-device copy of as many
bytes as the stage's own passes must touch (per half-edge the flag pass reads and writes 17, per candidate a round moves 32).
--check compares every array with tests/hull_ref/brute.py and the layout figures with the restatement (the cloud capped at
5 M points).
usage: python tests/tools/hull_bench.py [--reps 7] [--points 50000000] [--check] [--out profiles/oriented_boxes_bench.json]"""
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
from buildingsegment_amd import api, hulls, synth  # noqa: E402

STREAM = None  # the stream the context runs on
STAGES = ("ms_outlines", "ms_candidates", "ms_rounds", "ms_order", "ms_boxes")
LAYOUT = ("n_candidates", "rounds", "max_live")


def hull_cases():
    spec = importlib.util.spec_from_file_location("hull_cases", os.path.join(ROOT, "tests", "hull_ref", "cases.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["hull_cases"] = mod
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


def image_case(ctx, name, d_label, w, h, n_labels, reps, check):
    o, outline_ms, _ = timed(lambda: ctx.facet_outlines_dev(d_label.data_ptr(), 0, w, h, n_labels), reps)
    hl, whole, runs = timed(lambda: hulls.label_hulls_dev(ctx, d_label.data_ptr(), w, h, n_labels), reps)
    d_xy = torch.empty((max(hl.n_hull_vertices, 1), 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _, emit_ms, _ = timed(lambda: hulls.label_hulls_emit_dev(ctx, d_xy.data_ptr()), reps)
    nc, rounds = hl.info["n_candidates"], hl.info["rounds"]
    nbytes = 17 * o.n_half + 32 * nc * max(rounds, 1)
    row = {"case": name, "width": w, "height": h, "reps": reps, "labels": n_labels, "n_half": o.n_half, "n_rings": o.n_rings,
           "n_ok": hl.n_ok, "n_empty": hl.n_empty, "n_too_large": hl.n_too_large, "n_hull_vertices": hl.n_hull_vertices,
           "largest_hull": int(hl.n_hull.max()) if n_labels else 0, **{k: hl.info[k] for k in LAYOUT}, "bytes_own": nbytes,
           "label_hulls_count_dev_ms": stat(whole), "label_hulls_emit_dev_ms": stat(emit_ms),
           "facet_outlines_count_dev_ms": stat(outline_ms), "copy_own_ms": stat(copy_ms(nbytes, reps))}
    for k in STAGES:
        row[k] = stat([x.info[k] for x in runs])
    own = sum(row[k]["median"] for k in STAGES[1:])
    row["ms_own_stages_sum"] = round(own, 3)
    row["count_over_outlines"] = round(row["label_hulls_count_dev_ms"]["median"] / row["facet_outlines_count_dev_ms"]["median"], 3)
    row["own_over_outlines"] = round(own / row["facet_outlines_count_dev_ms"]["median"], 3)
    if check:
        cases = hull_cases()
        c = cases.case(d_label.cpu().numpy(), n_labels)
        hl.hull_xy = d_xy.cpu().numpy()[:hl.n_hull_vertices]
        diff = cases.brute.same(hl, cases.run_brute(c))
        row["equal_to_definition"] = diff is None
        if diff is not None:
            row["first_difference"] = diff
        row["layout_equal_to_restatement"] = {k: hl.info[k] for k in LAYOUT} == cases.run_ref(c).info
    print(json.dumps(row), flush=True)
    return row


def cloud_cases(ctx, xyz, d_xyz, d_plane, planes, ext, bin_, reps, check):
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
    f = ctx.roof_facets_dev(d_map.data_ptr(), d_roof.data_ptr(), d_top.data_ptr(), w, h, b.n_buildings, n_planes, d_facet.data_ptr())
    torch.cuda.synchronize()
    return [image_case(ctx, f"urban_{n}_bin{bin_}_building_map", d_map, w, h, b.n_buildings, reps, check),
            image_case(ctx, f"urban_{n}_bin{bin_}_facet_image", d_facet, w, h, f.n_facets, reps, check)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out_path = a.out or os.path.join(ROOT, "profiles", "oriented_boxes_bench_check.json" if a.check else "oriented_boxes_bench.json")
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
    rows = cloud_cases(ctx, xyz, d_xyz, d_plane, planes, ext, 100, a.reps, a.check)
    out = {"tool": "tests/tools/hull_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
