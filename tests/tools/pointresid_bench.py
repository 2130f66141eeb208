#!/usr/bin/env python3
"""Times the point residuals (bs_point_residuals_dev: rows, spans, lists, points) on urban at --points (bench.py's urban_50m
at the default) at bin 100 and bin 25, at tolerances of 1, 2 and 4 pixels, through the chain of tests/tools/polysolid_bench.py
in the same run.  HIP events on the context's stream, median of --reps after 2 warm-ups, with min and max.  The four phases
are the library's own event times and include what the host does between them (the reads of n_rows, n_items, the checks and
the result).  Every row is measured twice: with the cloud in input order and sorted by base pixel.  Beside them, measured in
the same run: bs_assign_buildings_dev on the same cloud (the existing one-gather pass over the points),
bs_model_raster_dev without images on the same state, and a device-to-device copy of the bytes the call touches (per point the
cloud twice, the plane, the three outputs, two offsets, and one list entry with its record; the lists themselves).  Per row
the figures themselves: bias, mean absolute residual and RMSE in millimetres over the inliers, the shares above and below the
clip of --clip-mm, and the plane agreement.
--check compares every per-point value and figure with the restatement tests/pointresid_ref (the cloud capped at 5 M points).
usage: python tests/tools/pointresid_bench.py [--reps 7] [--points 50000000] [--clip-mm 500] [--check]
       [--out profiles/point_residuals_bench.json]"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import simplify_bench as sbench  # noqa: E402  (the timer and the statistics)
from buildingsegment_amd import api, synth  # noqa: E402

STAGES = ("ms_rows", "ms_spans", "ms_lists", "ms_points")
TOLERANCES_PX = (1, 2, 4)


def pointresid_ref():
    spec = importlib.util.spec_from_file_location("pointresid_ref", os.path.join(ROOT, "tests", "pointresid_ref", "pointresid_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["pointresid_ref"] = mod
    spec.loader.exec_module(mod)
    return mod


def facet_image(ctx, xyz, d_xyz, d_plane, planes, ext, bin_, reps):
    """the chain of polysolid_bench.facet_image, which also keeps what this stage needs of it: the plane of every facet, and
    the time of the building assignment on the same cloud"""
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
    assign = lambda: ctx.assign_buildings_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), b, d_bidx.data_ptr(), bin=bin_, ground_th=th)  # noqa: E731
    _, assign_ms, _ = sbench.timed(assign, reps)
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
    return (d_facet, d_top, w, h, int(f.n_facets), np.ascontiguousarray(f.facet_building, np.int32),
            np.ascontiguousarray(f.facet_plane, np.int32), int(b.n_buildings), sbench.stat(assign_ms))


def sorted_by_pixel(d_xyz, d_plane, bin_, w):
    """the cloud and its planes ordered by base pixel"""
    key = (d_xyz[:, 1] // bin_).to(torch.int64) * w + (d_xyz[:, 0] // bin_).to(torch.int64)
    order = torch.argsort(key)
    del key
    return d_xyz[order].contiguous(), d_plane[order].contiguous()


def case(ctx, n, bin_, px, im, clouds, clip_mm, reps, check):
    d_facet, d_top, w, h, n_facets, facet_building, facet_plane, nb, assign_ms = im
    num, den = api.simplify_tolerance(px * bin_, bin_)
    t = ctx.outline_triangles_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h, n_facets, num, den)[0]
    d_out = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    _, raster_ms, _ = sbench.timed(lambda: ctx.model_raster_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h), reps)
    row = {"case": f"urban_{n}_bin{bin_}_tol{px}px", "points": n, "bin": bin_, "tolerance_px": px, "tol2": [num, den], "width": w,
           "height": h, "reps": reps, "facets": n_facets, "buildings": nb, "clip_mm": clip_mm, "n_triangles": t.n_triangles,
           "n_failed_labels": t.n_failed_labels, "assign_buildings_dev_ms": assign_ms,
           "model_raster_dev_without_images_ms": sbench.stat(raster_ms)}
    for order, (d_xyz, d_plane) in clouds.items():
        call = lambda: ctx.point_residuals_dev(d_xyz.data_ptr(), n, bin_, d_plane.data_ptr(), facet_plane, 2 * clip_mm,  # noqa: E731
                                               *[o.data_ptr() for o in d_out])
        r, whole, runs = sbench.timed(call, reps)
        row[f"point_residuals_dev_ms_{order}"] = sbench.stat(whole)
        for key in STAGES:
            row[f"{key}_{order}"] = sbench.stat([x.info[key] for x in runs])
    nbytes = n * (24 + 4 + 12 + 8 + 4 + 48) + 8 * r.n_items + 8 * w * h + 48 * t.n_triangles + 24 * r.n_rows
    f = api.point_fidelity_of(r, facet_building if n_facets else np.zeros(0, np.int32), nb)
    sq = sum((int(hi) << 32) + int(lo) for hi, lo in zip(r.sq_hi, r.sq_lo))
    ni, npts = max(r.total_in_points, 1), max(r.total_points, 1)
    row.update({"n_rows": r.n_rows, "n_items": r.n_items, "max_list": r.max_list, "n_empty_pixel": r.n_empty_pixel,
                "n_height_wide": r.n_height_wide, "covered_points": r.total_points, "n_uncovered": r.n_uncovered,
                "n_multi": r.n_multi, "inlier_share": round(r.total_in_points / npts, 5),
                "above_share": round(r.total_above / npts, 5), "below_share": round(r.total_below / npts, 5),
                "bias_mm": round(r.total_sum_r2 / 2 / ni, 3), "mean_abs_mm": round(r.total_sum_abs_r2 / 2 / ni, 3),
                "rmse_mm": round((sq / 4 / ni) ** 0.5, 3), "max_abs_mm": r.max_abs_r2_all / 2,
                "plane_share": round(r.total_plane_points / npts, 5),
                "plane_in_share": round(r.total_plane_in / max(r.total_plane_points, 1), 5),
                "buildings_with_points": int((f.points > 0).sum()), "touched_bytes": nbytes,
                "copy_of_touched_bytes_ms": sbench.stat(sbench.copy_ms(nbytes, reps))})
    if check:
        pref = pointresid_ref()
        d_xyz, d_plane = clouds["sorted"]
        gt, gc, _, _ = ctx.outline_triangles(d_facet.cpu().numpy(), d_top.cpu().numpy(), n_labels=n_facets, num=num, den=den)
        want = pref.point_residuals(gc, gt, n_facets, w, h, d_xyz.cpu().numpy(), bin_, d_plane.cpu().numpy(), facet_plane, 2 * clip_mm)
        r.label, r.r2, r.cover = (o.cpu().numpy() for o in d_out)
        diff = pref.same(r, want)
        row["equal_to_restatement"] = diff is None
        if diff is not None:
            row["first_difference"] = diff
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--clip-mm", type=int, default=500)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = "point_residuals_bench_check.json" if a.check else "point_residuals_bench.json"
    out_path = a.out or os.path.join(ROOT, "profiles", name)
    ctx = api.Context(0)
    sbench.STREAM = torch.cuda.Stream()
    ctx.set_stream(sbench.STREAM.cuda_stream)
    n = min(a.points, 5_000_000) if a.check else a.points
    xyz = synth.shift_to_origin(synth.urban(n, seed=4))  # bench.py's urban_50m at the default size
    n = len(xyz)
    print(f"urban: {n} points", file=sys.stderr, flush=True)
    ext = xyz.max(0).astype(np.int32)
    d_xyz = torch.from_numpy(xyz).cuda()
    d_plane = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.segment_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), api.default_params(k=15))
    planes = ctx.planes_fetch()
    print(f"segmented: {len(planes)} planes", file=sys.stderr, flush=True)
    rows = []
    for bin_ in (100, 25):
        im = facet_image(ctx, xyz, d_xyz, d_plane, planes, ext, bin_, a.reps)
        clouds = {"input": (d_xyz, d_plane), "sorted": sorted_by_pixel(d_xyz, d_plane, bin_, im[2])}
        torch.cuda.synchronize()
        for px in TOLERANCES_PX:
            rows.append(case(ctx, n, bin_, px, im, clouds, a.clip_mm, a.reps, a.check))
        del im, clouds
        torch.cuda.empty_cache()
    out = {"tool": "tests/tools/pointresid_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()
    if a.check and not all(r["equal_to_restatement"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
