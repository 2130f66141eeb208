#!/usr/bin/env python3
"""Measures the roof generalisation (bs_roof_generalise_dev) on urban at --points (bench.py's urban_50m at the default) at
bin 100 and bin 25, from bs_segment_dev -> buildings -> roofs in the same run (the chain of facet_bench.py), for four
parameter sets: merge_flat alone, min_pixels 16, min_pixels 64, and merge_flat with min_pixels 16.  Per set: facets and
edges in and out, rounds, the dtop figures, the phase times (the library's HIP events, median of --reps after 2 warm-ups),
and downstream the clean vertex count, the triangle count and the polygon-solid face count at a tolerance of one pixel
before and after.  Beside them, re-measured in the same run on the same image: the device phases of bs_solids_count_dev
plus bs_roof_facets_dev -- one evaluation contains one of each, so they are its yardstick.
--check compares every array with the restatement tests/generalise_ref (the cloud capped at 5 M points).
usage: python tests/tools/generalise_bench.py [--reps 5] [--points 50000000] [--check] [--out profiles/roof_generalise_bench.json]"""
import argparse
import importlib.util
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
torch.zeros(1, device="cuda")
from buildingsegment_amd import api, synth  # noqa: E402

SETS = (("merge_flat", dict(merge_flat=True)), ("min_pixels_16", dict(min_pixels=16)), ("min_pixels_64", dict(min_pixels=64)),
        ("merge_flat_min_pixels_16", dict(merge_flat=True, min_pixels=16)))
PHASES = ("ms_tops", "ms_facets", "ms_decide", "ms_apply", "ms_figures")
SOLID_PHASES = ("ms_tops", "ms_vertices", "ms_faces", "ms_figures", "ms_scans")
FACET_PHASES = ("ms_label", "ms_number", "ms_figures", "ms_edges")


def generalise_ref():
    spec = importlib.util.spec_from_file_location("generalise_ref", os.path.join(ROOT, "tests", "generalise_ref", "generalise_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def med(v):
    return round(float(np.median(v)), 3)


def repeat(fn, reps):
    outs = [fn() for _ in range(reps + 2)]
    return outs[2:]


def downstream(ctx, bmap, roofs, base_z, flat, bin_):
    """clean vertices, triangles and polygon-solid faces of a roof image at a tolerance of one pixel"""
    s = ctx.solids(bmap, roofs, base_z=base_z, flat=flat)
    rf = ctx.roof_structure(bmap, roofs, s)
    p, t, o, _ = ctx.building_model(rf, s, tolerance_mm=bin_)
    return {"facets": int(rf.n_facets), "clean_vertices": int(o.n_svertices), "triangles": int(t.n_triangles),
            "poly_solid_faces": int(p.n_faces), "poly_solid_vertices": int(p.n_vertices), "open_buildings": int(p.n_open_buildings)}


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
    tabs = (normal, center, r.z_min, r.z_max, bin_, base_z, flat)
    d_top = torch.empty((h, w, 4), dtype=torch.int32, device="cuda")
    d_facet = torch.empty((h, w), dtype=torch.int32, device="cuda")
    d_out = torch.empty((h, w), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # the yardstick: the device phases of one solids count and one facet pass on the same image
    sol = repeat(lambda: ctx.solids_dev(d_map.data_ptr(), d_roof.data_ptr(), w, h, *tabs, d_top=d_top.data_ptr()), reps)
    fac = repeat(lambda: ctx.roof_facets_dev(d_map.data_ptr(), d_roof.data_ptr(), d_top.data_ptr(), w, h, b.n_buildings, n_planes,
                                             d_facet.data_ptr()), reps)
    yard = med([sum(x.info[k] for k in SOLID_PHASES) for x in sol]) + med([sum(x.info[k] for k in FACET_PHASES) for x in fac])
    bmap, roof = d_map.cpu().numpy(), d_roof.cpu().numpy()
    roofs = SimpleNamespace(roof=roof, normal=normal, center=center, z_min=r.z_min, z_max=r.z_max, bin=bin_)
    before = downstream(ctx, bmap, roofs, base_z, flat, bin_)
    row = {"case": f"urban_{n}_bin{bin_}", "points": n, "bin": bin_, "width": w, "height": h, "reps": reps,
           "buildings": b.n_buildings, "planes": n_planes, "solids_ms": med([sum(x.info[k] for k in SOLID_PHASES) for x in sol]),
           "solids_tops_ms": med([x.info["ms_tops"] for x in sol]),
           "roof_facets_ms": med([sum(x.info[k] for k in FACET_PHASES) for x in fac]), "yardstick_ms": round(yard, 3),
           "downstream_before": before, "sets": []}
    for name, par in SETS:
        runs = repeat(lambda: ctx.generalise_roofs_dev(d_map.data_ptr(), d_roof.data_ptr(), w, h, *tabs, d_out.data_ptr(), **par),
                      reps)
        g = runs[-1]
        evals = g.rounds + 1
        ms = {k: med([x.info[k] for x in runs]) for k in PHASES}
        per_eval = round((ms["ms_tops"] + ms["ms_facets"] + ms["ms_decide"]) / evals, 3)
        new = d_out.cpu().numpy()
        s = {"set": name, "params": par, "rounds": g.rounds, "converged": g.converged, "facets_in": g.n_facets_in,
             "facets_out": g.n_facets_out, "edges_in": g.n_edges_in, "edges_out": g.n_edges_out, "flat_in": g.n_flat_in,
             "flat_out": g.n_flat_out, "small_in": g.n_small_in, "small_out": g.n_small_out,
             "eval_facets": g.eval_facets.tolist(), "eval_movers": g.eval_movers.tolist(),
             "eval_longest_chain": g.eval_longest_chain.tolist(), "pixels_changed": g.pixels_changed,
             "pixels_roofed": g.pixels_roofed, "sum_abs_dtop": int(g.building_sum_abs_dtop.sum()),
             "max_abs_dtop": int(g.building_max_abs_dtop.max(initial=0)),
             "mean_abs_dtop_per_changed_corner": round(float(g.building_sum_abs_dtop.sum()) / max(4 * g.pixels_changed, 1), 2),
             **ms, "ms_per_evaluation": per_eval, "evaluation_over_yardstick": round(per_eval / yard, 3),
             "dominant_phase": max(PHASES, key=lambda k: ms[k]),
             "downstream_after": downstream(ctx, bmap, SimpleNamespace(**{**roofs.__dict__, "roof": new}), base_z, flat, bin_)}
        if check:
            gr = generalise_ref()
            g.roof = new
            want = gr.generalise(bmap, roof, b.n_buildings, normal, center, r.z_min, r.z_max, bin_, base_z, flat,
                                 **{"min_pixels": 0, "merge_flat": False, **par})
            diff = gr.same(g, want)
            s["equal_to_restatement"] = diff is None
            if diff is not None:
                s["first_difference"] = diff
        row["sets"].append(s)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roof_generalise_bench.json"))
    a = ap.parse_args()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
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
    out = {"tool": "tests/tools/generalise_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
