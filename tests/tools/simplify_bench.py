#!/usr/bin/env python3
"""Times the simplified outlines (bs_simple_outlines_count_dev: the plain count, nodes, placing, arcs, rounds, rings;
bs_simple_outlines_emit_dev) on urban at --points (bench.py's urban_50m at the default) at bin 100 and bin 25 and at
tolerances of 0, 1 and 2 pixels, from bs_segment_dev -> buildings -> roofs -> solids -> facets in the same run.  HIP events
on the context's stream, median of --reps after 2 warm-ups, with min and max.  Beside them, re-measured in the same run on
the same image: bs_facet_outlines_count_dev, and a device-to-device copy of as many bytes as one round must touch (72 per
node: the segment read three times and written once, c^2 written once and read once, the next round's maximum and tie
reset; the gathers of the segment ends and of the segment's maximum and tie are not counted).
--check compares every array with the restatement tests/simplify_ref (the cloud capped at 5 M points).
usage: python tests/tools/simplify_bench.py [--reps 7] [--points 50000000] [--check] [--out profiles/outline_simplify_bench.json]"""
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
STAGES = ("ms_outlines", "ms_nodes", "ms_placing", "ms_arcs", "ms_rounds", "ms_rings")
ROUND_BATCH = 4      # rounds between two reads of the "kept something" words (bs_simplify.hip)
ROUND_BYTES = 72     # per node and round, see above
TOLERANCES_PX = (0, 1, 2)


def simplify_ref():
    spec = importlib.util.spec_from_file_location("simplify_ref", os.path.join(ROOT, "tests", "simplify_ref", "simplify_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["simplify_ref"] = mod
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


def facet_image(ctx, xyz, d_xyz, d_plane, planes, ext, bin_):
    """the chain up to the facets: returns (d_facet, d_top, w, h, n_facets); the tensors stay alive with the caller"""
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
    f = ctx.roof_facets_dev(d_map.data_ptr(), d_roof.data_ptr(), d_top.data_ptr(), w, h, b.n_buildings, n_planes,
                            d_facet.data_ptr())
    torch.cuda.synchronize()
    return d_facet, d_top, w, h, int(f.n_facets)


def tolerance_case(ctx, n, bin_, px, d_facet, d_top, w, h, n_facets, plain_ms, reps, check):
    num, den = api.simplify_tolerance(px * bin_, bin_)
    count = lambda: ctx.simplified_outlines_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h, n_facets, num, den)  # noqa: E731
    (s, plain), whole, runs = timed(count, reps)
    nv = s.n_svertices
    d_xy = torch.empty((nv, 2), dtype=torch.int32, device="cuda")
    d_z, d_right = (torch.empty((nv,), dtype=torch.int32, device="cuda") for _ in range(2))
    d_flag = torch.empty((nv,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    emit = lambda: ctx.simplified_outlines_emit_dev(d_xy.data_ptr(), d_z.data_ptr(), d_right.data_ptr(), d_flag.data_ptr())  # noqa: E731
    _, emit_ms, _ = timed(emit, reps)
    launched = (s.rounds // ROUND_BATCH + 1) * ROUND_BATCH  # whole batches until a round keeps nothing
    bytes_round = ROUND_BYTES * s.n_nodes
    row = {"case": f"urban_{n}_bin{bin_}_tol{px}px", "points": n, "bin": bin_, "tolerance_px": px, "tol2": [num, den],
           "width": w, "height": h, "reps": reps, "facets": n_facets, "n_half": plain.n_half, "n_rings": plain.n_rings,
           "n_nodes": s.n_nodes, "n_junction_nodes": s.n_junction_nodes, "n_arcs": s.n_arcs, "max_arc_nodes": s.max_arc_nodes,
           "rounds": s.rounds, "rounds_launched": launched, "vertices_before": plain.n_vertices, "vertices_after": nv,
           "vertices_ratio": round(nv / max(plain.n_vertices, 1), 4), "rings_of_2_vertices": int((s.s_ring_vertices < 3).sum()),
           "bytes_round": bytes_round, "simple_outlines_count_dev_ms": stat(whole), "simple_outlines_emit_dev_ms": stat(emit_ms),
           "facet_outlines_count_dev_ms": stat(plain_ms), "copy_round_ms": stat(copy_ms(bytes_round, reps))}
    for k in STAGES:
        row[k] = stat([x[0].info[k] for x in runs])
    row["ms_stages_sum"] = round(sum(row[k]["median"] for k in STAGES), 3)
    row["dominant_stage"] = max(STAGES, key=lambda k: row[k]["median"])
    row["ms_per_round_launched"] = round(row["ms_rounds"]["median"] / launched, 4)
    row["copy_over_round"] = round(row["copy_round_ms"]["median"] / max(row["ms_per_round_launched"], 1e-9), 3)
    row["count_over_plain_count"] = round(row["simple_outlines_count_dev_ms"]["median"] /
                                          row["facet_outlines_count_dev_ms"]["median"], 3)
    if check:
        sref = simplify_ref()
        s.sxy, s.sz, s.s_right, s.s_flag = (t.cpu().numpy() for t in (d_xy, d_z, d_right, d_flag))
        wp, want = sref.simplify(d_facet.cpu().numpy(), d_top.cpu().numpy(), n_facets, num, den)
        diff = sref.same(s, want)
        row["equal_to_restatement"] = diff is None
        if diff is not None:
            row["first_difference"] = diff
        row["plain_equal_to_restatement"] = all(
            np.array_equal(np.asarray(getattr(plain, f), np.int64), np.asarray(getattr(wp, f), np.int64))
            for f in sref.orf.brute.FIELDS if f not in ("xy", "z"))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = "outline_simplify_bench_check.json" if a.check else "outline_simplify_bench.json"
    out_path = a.out or os.path.join(ROOT, "profiles", name)
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
        d_facet, d_top, w, h, n_facets = facet_image(ctx, xyz, d_xyz, d_plane, planes, ext, bin_)
        _, plain_ms, _ = timed(lambda: ctx.facet_outlines_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h, n_facets), a.reps)
        for px in TOLERANCES_PX:
            rows.append(tolerance_case(ctx, n, bin_, px, d_facet, d_top, w, h, n_facets, plain_ms, a.reps, a.check))
        del d_facet, d_top
        torch.cuda.empty_cache()
    out = {"tool": "tests/tools/simplify_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
