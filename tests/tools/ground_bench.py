#!/usr/bin/env python3
"""Times the ground stage (bs_ground_dev: low, the K steps, the points) on the cloud of tests/tools/terrain_bench.py:
synth.urban at --points lifted onto its rising sheet.  HIP events on the context's stream, median of --reps after 2 warm-ups,
with min and max; the phases are the library's own event times and include the host's two waits.  Rows:
  stage      the whole call and its phases at cell 500 and 100 (default parameters), next to bs_terrain_dev,
             bs_assign_buildings_dev and a device-to-device copy of the 12 bytes per point that a pass over the points reads
  radius     one step at r = 1 and at r = 255 on the cell-100 lattice: does a step cost more at a larger radius?
  consumers  bs_grid_picture_dev, bs_assign_buildings_dev and bs_roofs_dev with the ground model off and on, alternated call by
             call in one process
  scenes     the dense tilted scenes of tests/ground_ref: buildings found and IoU per box with ground=None and ground={}
--consumers times the three consumers alone (switch off; on as well where the library has the switch) and APPENDS its row to
the output file under --label; with --package-root it does so for the package of another checkout (the parent commit's),
so that two libraries can be alternated process by process on one box.
--check compares every array and figure with the restatement tests/ground_ref (the cloud capped at 2 M points).
usage: python tests/tools/ground_bench.py [--reps 7] [--points 10000000] [--check] [--consumers --label NAME
       [--package-root DIR]] [--out profiles/ground_bench.json]"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def _package_root():
    for i, a in enumerate(sys.argv):
        if a == "--package-root" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
    return ROOT


sys.path.insert(0, HERE)
sys.path.insert(0, _package_root())
from buildingsegment_amd import api, synth  # noqa: E402  (first: the tools below put this checkout in front of the path)
import simplify_bench as sbench  # noqa: E402  (the timer and the statistics)
import terrain_bench as tbench  # noqa: E402  (the cloud)

BIN = 100


def ground_cases():
    spec = importlib.util.spec_from_file_location("ground_cases", os.path.join(ROOT, "tests", "ground_ref", "cases.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ground_cases"] = mod
    spec.loader.exec_module(mod)
    return mod


def med(v):
    return float(np.median(v))


def stage_row(ctx, d_xyz, n, ext, cell, reps, radius=None):
    p = api.ground_params(cell=cell, radius=radius)
    w, h = api.grid_dims(ext, cell)
    d_low, d_dtm = (torch.empty((h, w), dtype=torch.int32, device="cuda") for _ in range(2))
    d_step = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    d_hag = torch.empty(n, dtype=torch.int32, device="cuda")
    d_cls = torch.empty(n, dtype=torch.uint8, device="cuda")
    call = lambda: ctx.ground_dev(d_xyz.data_ptr(), n, ext, p, d_low=d_low.data_ptr(), d_dtm=d_dtm.data_ptr(),  # noqa: E731
                                  d_step=d_step.data_ptr(), d_hag=d_hag.data_ptr(), d_class=d_cls.data_ptr())
    g, whole, runs = sbench.timed(call, reps)
    row = {"cell": cell, "width": w, "height": h, "radius": p["radius"], "threshold": g.threshold, "ground_dev_ms": sbench.stat(whole)}
    for key in ("ms_low", "ms_open", "ms_points"):
        row[key] = sbench.stat([x.info[key] for x in runs])
    row["ms_step"] = [sbench.stat([x.info["ms_step"][k] for x in runs]) for k in range(g.n_steps)]
    for key in ("step_pixels", "n_ground_pixels", "n_object_pixels", "n_empty_pixels", "n_filled_pixels", "n_ground_points",
                "n_low_points", "n_object_points", "dtm_min", "dtm_max", "hag_min", "hag_max", "sum_hag_ground"):
        row[key] = getattr(g, key)
    arrays = dict(low=d_low, dtm=d_dtm, step=d_step, hag=d_hag, cls=d_cls)
    return row, g, arrays


def chain(ctx, d_xyz, n, ext):
    """the 2-D branch and the labels the roofs need, on the device: everything the three consumers take"""
    d_map, b, th, w, h = tbench.building_map(ctx, d_xyz, n, ext)
    nb = b.n_buildings
    d_bidx = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.assign_buildings_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), b, d_bidx.data_ptr(), bin=BIN, ground_th=th)
    d_plane = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.segment_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), api.default_params(k=15))
    planes = ctx.planes_fetch()
    n_planes = len(planes)
    normal = np.array([p.normal for p in planes], np.float64).reshape(n_planes, 3)
    center = np.array([p.center for p in planes], np.int32).reshape(n_planes, 3)
    votes = ctx.plane_buildings_dev(d_plane.data_ptr(), d_bidx.data_ptr(), n, n_planes, nb)
    home = api.roof_homes(normal, votes.plane_building, votes.votes_in, votes.votes_total)
    d_img = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    d_roof = torch.empty((h, w), dtype=torch.int32, device="cuda")
    calls = {
        "grid_picture_dev": lambda: ctx.grid_picture_dev(d_xyz.data_ptr(), n, ext, d_img.data_ptr(), bin=BIN),
        "assign_buildings_dev": lambda: ctx.assign_buildings_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), b, d_bidx.data_ptr(), bin=BIN,
                                                                 ground_th=th),
        "roofs_dev": lambda: ctx.roofs_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), w, h, d_plane.data_ptr(), home, normal, center,
                                           d_roof.data_ptr(), 0, 0, bin=BIN, ground_th=th),
    }
    keep = (d_map, d_bidx, d_plane, d_img, d_roof)
    return calls, keep, {"buildings": nb, "planes": n_planes, "ground_th": float(th), "width": w, "height": h}


def consumers_row(ctx, d_xyz, n, ext, reps, model):
    """the three consumers with the switch off and (model = (device dtm tensor, cell, min_height) or None) on, alternated"""
    calls, keep, row = chain(ctx, d_xyz, n, ext)
    modes = ("off", "on") if model is not None else ("off",)
    for name, fn in calls.items():
        ms = {m: [] for m in modes}
        for it in range(reps + 2):  # (two warm-ups of either mode)
            for mode in modes:
                if model is not None:
                    ctx.set_ground_model((model[0].data_ptr(), model[0].shape[1], model[0].shape[0]) if mode == "on" else None,
                                         model[1], model[2], device=mode == "on")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(sbench.STREAM)
                fn()
                e1.record(sbench.STREAM)
                e1.synchronize()
                if it >= 2:
                    ms[mode].append(e0.elapsed_time(e1))
        for mode in modes:
            row[f"{name}_ms_switch_{mode}"] = sbench.stat(ms[mode])
    if model is not None:
        ctx.set_ground_model(None)
    del keep
    return row


def scenes_rows(ctx):
    cases = ground_cases()
    truth = cases.slope_map(BIN)
    rows = []
    for rise in (0, 100, 200):
        xyz = cases.scene(rise)
        _, b0 = ctx.buildings(xyz, bin=BIN)
        _, b1, g = ctx.buildings(xyz, bin=BIN, ground={})
        rows.append({"mode": "scene", "rise_mm_per_m": rise, "points": len(xyz), "ground_th": b0.ground_th,
                     "scalar_buildings": b0.n_buildings, "scalar_iou": [round(s, 4) for s in cases.gref.box_scores(b0.map, truth)],
                     "model_buildings": b1.n_buildings, "model_iou": [round(s, 4) for s in cases.gref.box_scores(b1.map, truth)],
                     "ground_ms": {k: round(v, 4) for k, v in g.info.items() if k != "ms_step"}})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--consumers", action="store_true")
    ap.add_argument("--label", default="this")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out_path = a.out or os.path.join(ROOT, "profiles", "ground_bench_check.json" if a.check else "ground_bench.json")
    ctx = api.Context(0)
    sbench.STREAM = torch.cuda.Stream()
    ctx.set_stream(sbench.STREAM.cuda_stream)
    n_urban = min(a.points, 2_000_000) if a.check else a.points
    xyz, n_sheet = tbench.with_sheet(ctx, synth.shift_to_origin(synth.urban(n_urban, seed=3)))
    n = len(xyz)
    print(f"urban {n_urban} + sheet {n_sheet} = {n} points", file=sys.stderr, flush=True)
    ext = xyz.max(0).astype(np.int32)
    d_xyz = torch.from_numpy(xyz).cuda()
    case = f"urban_{n_urban}_sheet"
    has_switch = hasattr(ctx, "set_ground_model")
    if a.consumers:
        model = None
        if has_switch:
            _, g, arrays = stage_row(ctx, d_xyz, n, ext, 500, 1)
            model = (arrays["dtm"], g.cell, g.min_height)
        row = dict({"mode": "consumers_process", "label": a.label, "case": case, "points": n, "reps": a.reps, "pid": os.getpid(),
                    "library": os.path.relpath(api._lib.LIB_PATH, ROOT)},
                   **consumers_row(ctx, d_xyz, n, ext, a.reps, model))
        print(json.dumps(row), flush=True)
        doc = json.load(open(out_path)) if os.path.exists(out_path) else {"tool": "tests/tools/ground_bench.py", "rows": []}
        doc["rows"].append(row)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
        ctx.close()
        return
    rows, ok = [], True
    models = {}
    for cell in (500, 100):
        row, g, arrays = stage_row(ctx, d_xyz, n, ext, cell, a.reps)
        row = dict({"mode": "stage", "case": case, "points": n, "sheet_points": n_sheet, "reps": a.reps}, **row)
        if a.check:
            cases = ground_cases()
            want = cases.gref.ground(xyz, ext, api.ground_params(cell=cell))
            diff = next((k for k in ("threshold", "step_pixels") + cases.gref.FIGURES if getattr(g, k) != getattr(want, k)), None)
            diff = diff or next((k for k, t in arrays.items() if not np.array_equal(t.cpu().numpy(), getattr(want, k))), None)
            row["equal_to_restatement"] = diff is None
            if diff is not None:
                row["first_difference"], ok = diff, False
        models[cell] = (arrays["dtm"], g.cell, g.min_height)
        rows.append(row)
        print(json.dumps(row), flush=True)
    # beside the stage, on the same cloud
    d_map, b, th, w, h = tbench.building_map(ctx, d_xyz, n, ext)
    d_bidx = torch.empty(n, dtype=torch.int32, device="cuda")
    _, assign_ms, _ = sbench.timed(lambda: ctx.assign_buildings_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), b, d_bidx.data_ptr(), bin=BIN,
                                                                     ground_th=th), a.reps)
    _, terrain_ms, _ = sbench.timed(lambda: ctx.terrain_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), w, h, b.n_buildings, bin=BIN,
                                                            fallback_z=int(th)), a.reps)
    copy_ms = sbench.copy_ms(12 * n, a.reps)
    row = {"mode": "beside", "case": case, "points": n, "assign_buildings_dev_ms": sbench.stat(assign_ms),
           "terrain_dev_ms": sbench.stat(terrain_ms), "copy_12_bytes_per_point_ms": sbench.stat(copy_ms)}
    for r in rows:
        row[f"ground_cell{r['cell']}_over_assign"] = round(r["ground_dev_ms"]["median"] / max(med(assign_ms), 1e-9), 3)
        row[f"low_pass_cell{r['cell']}_over_copy"] = round(r["ms_low"]["median"] / max(med(copy_ms), 1e-9), 3)
    del d_map, d_bidx
    rows.append(row)
    print(json.dumps(row), flush=True)
    # one step against its radius
    for r in (1, 255):
        row, g, _ = stage_row(ctx, d_xyz, n, ext, 100, a.reps, radius=[r])
        rows.append({"mode": "radius", "case": case, "cell": 100, "width": row["width"], "height": row["height"], "radius": r,
                     "one_step_ms": row["ms_step"][0], "ms_open": row["ms_open"]})
        print(json.dumps(rows[-1]), flush=True)
    if not a.check:
        rows.append(dict({"mode": "consumers", "case": case, "points": n, "reps": a.reps, "model_cell": 500},
                         **consumers_row(ctx, d_xyz, n, ext, a.reps, models[500])))
        print(json.dumps(rows[-1]), flush=True)
    del d_xyz, models
    rows += scenes_rows(ctx)
    for r in rows[-3:]:
        print(json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump({"tool": "tests/tools/ground_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    ctx.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
