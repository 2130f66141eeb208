#!/usr/bin/env python3
"""Times the terrain stage (bs_terrain_dev: ring, points, pixels, pick) on synth.urban at --points plus a tilted ground sheet
of its own: urban has no ground points, so a sheet at 200 mm spacing that rises 1 % along x is laid under it and removed
under the roofs (the pixels of the building map of urban's own raster), as the gabled scene of tests/roof_ref does.  HIP
events on the context's stream, median of --reps after 2 warm-ups, with min and max; the four phases are the library's own
event times and include the host's two waits.  Beside them, measured in the same run on the same cloud and map:
bs_assign_buildings_dev (the closest existing pass: one read of every point, one image gather), and bs_solids_count_dev over
the roofs of the same chain with the per-building bases on and off, alternated call by call.
--check compares every image and figure with the restatement tests/terrain_ref (the cloud capped at 2 M points).
usage: python tests/tools/terrain_bench.py [--reps 7] [--points 10000000] [--ring 10] [--check] [--out profiles/terrain_bench.json]"""
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

STAGES = ("ms_ring", "ms_points", "ms_pixels", "ms_pick")
BIN = 100
SHEET_SPACING = 200
SHEET_RISE = 100  # 1 mm up per 100 mm along x


def terrain_ref():
    spec = importlib.util.spec_from_file_location("terrain_ref", os.path.join(ROOT, "tests", "terrain_ref", "terrain_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["terrain_ref"] = mod
    spec.loader.exec_module(mod)
    return mod


def building_map(ctx, d_xyz, n, ext):
    """raster -> footprints -> building map on the device: (d_map, Buildings, ground_th, w, h)"""
    w, h = api.grid_dims(ext, BIN)
    d_img = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    th = ctx.grid_picture_dev(d_xyz.data_ptr(), n, ext, d_img.data_ptr(), bin=BIN)
    d_mask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    ctx.footprints_dev(d_img.data_ptr(), w, h, d_mask=d_mask.data_ptr())
    d_map = torch.empty((h, w), dtype=torch.int32, device="cuda")
    b = ctx.building_map_dev(d_mask.data_ptr(), w, h, d_map.data_ptr())
    torch.cuda.synchronize()
    return d_map, b, th, w, h


def with_sheet(ctx, urban):
    """urban lifted onto a tilted sheet: the sheet's points outside the buildings of urban's own map, urban's points raised
    by the sheet's height where they stand"""
    ext = urban.max(0).astype(np.int32)
    d_xyz = torch.from_numpy(urban).cuda()
    d_map, _, _, w, h = building_map(ctx, d_xyz, len(urban), ext)
    bmap = d_map.cpu().numpy()
    del d_xyz, d_map
    gx, gy = np.meshgrid(np.arange(0, int(ext[0]) + 1, SHEET_SPACING, dtype=np.int32),
                         np.arange(0, int(ext[1]) + 1, SHEET_SPACING, dtype=np.int32), indexing="ij")
    gx, gy = gx.ravel(), gy.ravel()
    keep = bmap[np.minimum(gy // BIN, h - 1), np.minimum(gx // BIN, w - 1)] < 0
    sheet = np.stack([gx[keep], gy[keep], gx[keep] // SHEET_RISE], 1).astype(np.int32)
    lifted = urban.copy()
    lifted[:, 2] += lifted[:, 0] // SHEET_RISE
    rng = np.random.default_rng(5)
    xyz = np.concatenate([lifted, sheet])
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))]), len(sheet)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--ring", type=int, default=10)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out_path = a.out or os.path.join(ROOT, "profiles", "terrain_bench_check.json" if a.check else "terrain_bench.json")
    ctx = api.Context(0)
    sbench.STREAM = torch.cuda.Stream()
    ctx.set_stream(sbench.STREAM.cuda_stream)
    n_urban = min(a.points, 2_000_000) if a.check else a.points
    xyz, n_sheet = with_sheet(ctx, synth.shift_to_origin(synth.urban(n_urban, seed=3)))
    n = len(xyz)
    print(f"urban {n_urban} + sheet {n_sheet} = {n} points", file=sys.stderr, flush=True)
    ext = xyz.max(0).astype(np.int32)
    d_xyz = torch.from_numpy(xyz).cuda()
    d_map, b, th, w, h = building_map(ctx, d_xyz, n, ext)
    nb = b.n_buildings
    # the stage, and the assignment pass on the same cloud and map
    d_img = [torch.empty((h, w), dtype=dt, device="cuda") for dt in (torch.int32, torch.uint8, torch.int32)]
    call = lambda: ctx.terrain_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), w, h, nb, bin=BIN, ring=a.ring, fallback_z=int(th),  # noqa: E731
                                   d_owner=d_img[0].data_ptr(), d_dist=d_img[1].data_ptr(), d_low=d_img[2].data_ptr())
    t, whole, runs = sbench.timed(call, a.reps)
    d_bidx = torch.empty(n, dtype=torch.int32, device="cuda")
    assign = lambda: ctx.assign_buildings_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), b, d_bidx.data_ptr(), bin=BIN, ground_th=th)  # noqa: E731
    _, assign_ms, _ = sbench.timed(assign, a.reps)
    row = {"case": f"urban_{n_urban}_sheet_bin{BIN}_ring{a.ring}", "points": n, "sheet_points": n_sheet, "width": w, "height": h,
           "buildings": nb, "reps": a.reps, "ground_th": float(th), "terrain_dev_ms": sbench.stat(whole),
           "assign_buildings_dev_ms": sbench.stat(assign_ms),
           "terrain_over_assign": round(float(np.median(whole)) / max(float(np.median(assign_ms)), 1e-9), 3),
           "points_pass_over_assign": round(float(np.median([x.info["ms_points"] for x in runs])) / max(float(np.median(assign_ms)), 1e-9), 3)}
    for key in STAGES:
        row[key] = sbench.stat([x.info[key] for x in runs])
    g = t.ground[t.status == 0]
    row.update({"rounds_used": t.rounds_used, "n_ring_pixels": t.n_ring_pixels, "n_ground_pixels": t.n_ground_pixels,
                "n_ring_points": t.n_ring_points, "ring_point_share": round(t.n_ring_points / n, 5), "n_fallback": t.n_fallback,
                "ground_min_mm": int(g.min()) if len(g) else None, "ground_max_mm": int(g.max()) if len(g) else None,
                "ground_below_ground_th": int((g < th).sum())})
    # the solids of the same chain with the switch off and on, alternated call by call
    d_plane = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.segment_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), api.default_params(k=15))
    planes = ctx.planes_fetch()
    n_planes = len(planes)
    normal = np.array([p.normal for p in planes], np.float64).reshape(n_planes, 3)
    center = np.array([p.center for p in planes], np.int32).reshape(n_planes, 3)
    votes = ctx.plane_buildings_dev(d_plane.data_ptr(), d_bidx.data_ptr(), n, n_planes, nb)
    home = api.roof_homes(normal, votes.plane_building, votes.votes_in, votes.votes_total)
    d_roof = torch.empty((h, w), dtype=torch.int32, device="cuda")
    r = ctx.roofs_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), w, h, d_plane.data_ptr(), home, normal, center, d_roof.data_ptr(), 0, 0,
                      bin=BIN, ground_th=th)
    b.ground_th = th  # (the scalar base of the pipeline: Context.buildings sets it the same way)
    base_z, flat = api._solid_defaults(b, None, None)
    solids = lambda: ctx.solids_dev(d_map.data_ptr(), d_roof.data_ptr(), w, h, normal, center, r.z_min, r.z_max, BIN, base_z, flat)  # noqa: E731
    ms = {"off": [], "on": []}
    vol = {}
    for it in range(a.reps + 2):  # (two warm-ups of either mode)
        for mode in ("off", "on"):
            ctx.set_building_bases(t.ground if mode == "on" and nb else None)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(sbench.STREAM)
            s = solids()
            e1.record(sbench.STREAM)
            e1.synchronize()
            if it >= 2:
                ms[mode].append(e0.elapsed_time(e1))
            vol[mode] = int(s.total_volume6)
    ctx.set_building_bases(None)
    row.update({"planes": n_planes, "solids_count_dev_ms_switch_off": sbench.stat(ms["off"]),
                "solids_count_dev_ms_switch_on": sbench.stat(ms["on"]), "total_volume6_switch_off": vol["off"],
                "total_volume6_switch_on": vol["on"]})
    if a.check:
        tref = terrain_ref()
        want = tref.terrain(xyz, BIN, d_map.cpu().numpy(), nb, a.ring, (1, 2), 8, int(th))
        t.owner, t.dist, t.low = (x.cpu().numpy() for x in d_img)
        diff = tref.same(t, want)
        row["equal_to_restatement"] = diff is None
        if diff is not None:
            row["first_difference"] = diff
    print(json.dumps(row), flush=True)
    with open(out_path, "w") as f:
        json.dump({"tool": "tests/tools/terrain_bench.py", "device": torch.cuda.get_device_name(0), "rows": [row]}, f, indent=1)
    ctx.close()
    if a.check and not row["equal_to_restatement"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
