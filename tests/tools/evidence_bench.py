#!/usr/bin/env python3
"""Times the roof evidence (bs_roof_evidence_dev: the counts pass over the points, the window kernel) on the cloud of
tests/tools/ground_bench.py -- synth.urban at --points lifted onto its rising sheet -- with the labels of bs_segment_dev and
the plane table of bs_plane_fit_dev -> bs_plane_quality at --max-rms-mm.  (On this synthetic cloud the grower's planes carry
stragglers from all over the tile and none passes the default 100 mm -- the row says how many would -- so the tool's default
lets every fitted plane count: the screen then has something to keep and the footprints under it something to trace.  The
counts pass does the same work either way.)  HIP events on the context's stream, median of --reps after 2
warm-ups, with min and max; the phases are the library's own event times and include the host's two waits.  Rows:
  stage       the whole call and its two phases at the defaults (r = 3), next to bs_assign_buildings_dev and a
              device-to-device copy of the 12 bytes per point that a pass over the points reads
  radius      the window kernel at r = 0, 3 and 15: does it cost more at a larger radius?
  order       the counts pass on the cloud as it is (shuffled) and on the same cloud sorted by pixel (scan order, where the
              waves add once per distinct pixel)
  footprints  bs_footprints_dev with the footprint screen off and on, alternated call by call in one process
--footprints times bs_footprints_dev alone (switch off; on as well where the library has the switch) and APPENDS its row to
the output file under --label; with --package-root it does so for the package of another checkout (the parent commit's), so
that two libraries can be alternated process by process on one box.
--check compares every image and figure with the restatement tests/evidence_ref (the cloud capped at 2 M points).
usage: python tests/tools/evidence_bench.py [--reps 7] [--points 10000000] [--max-rms-mm 32767] [--check] [--footprints --label NAME
       [--package-root DIR]] [--out profiles/roof_evidence_bench.json]"""
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
IMAGES = ("keep", "above", "planar", "win_above", "win_planar")


def evidence_cases():
    spec = importlib.util.spec_from_file_location("evidence_cases", os.path.join(ROOT, "tests", "evidence_ref", "cases.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["evidence_cases"] = mod
    spec.loader.exec_module(mod)
    return mod


def med(v):
    return float(np.median(v))


def stage_row(ctx, d_xyz, n, d_plane, n_planes, ok, ext, th, reps, **kw):
    p = api.evidence_params(**kw)
    w, h = api.grid_dims(ext, BIN)
    outs = {"keep": torch.empty((h, w), dtype=torch.uint8, device="cuda")}
    outs.update({k: torch.empty((h, w), dtype=torch.int32, device="cuda") for k in IMAGES[1:]})
    call = lambda: ctx.roof_evidence_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), n_planes, ext, outs["keep"].data_ptr(), ok,  # noqa: E731
                                         BIN, th, p, **{"d_" + k: outs[k].data_ptr() for k in IMAGES[1:]})
    e, whole, runs = sbench.timed(call, reps)
    row = {"r": p["r"], "width": w, "height": h, "roof_evidence_dev_ms": sbench.stat(whole)}
    for key in ("ms_counts", "ms_window"):
        row[key] = sbench.stat([x.info[key] for x in runs])
    for key in ("n_counted", "n_planar", "n_pixels", "pixels_kept", "pixels_rejected", "pixels_thin", "max_window"):
        row[key] = getattr(e, key)
    return row, e, outs


def footprints_row(ctx, d_img, w, h, d_keep, reps):
    """bs_footprints_dev with the screen off and (d_keep: a device keep image, or None) on, alternated"""
    modes = ("off", "on") if d_keep is not None else ("off",)
    ms = {m: [] for m in modes}
    found = {}
    for it in range(reps + 2):  # (two warm-ups of either mode)
        for mode in modes:
            if d_keep is not None:
                ctx.set_footprint_screen((d_keep.data_ptr(), w, h) if mode == "on" else None, device=mode == "on")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(sbench.STREAM)
            fp = ctx.footprints_dev(d_img.data_ptr(), w, h)
            e1.record(sbench.STREAM)
            e1.synchronize()
            found[mode] = len(fp.contours)
            if it >= 2:
                ms[mode].append(e0.elapsed_time(e1))
    if d_keep is not None:
        ctx.set_footprint_screen(None)
    row = {"width": w, "height": h}
    for mode in modes:
        row[f"footprints_dev_ms_screen_{mode}"] = sbench.stat(ms[mode])
        row[f"contours_screen_{mode}"] = found[mode]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--max-rms-mm", type=int, default=32767)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--footprints", action="store_true")
    ap.add_argument("--label", default="this")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out_path = a.out or os.path.join(ROOT, "profiles", "roof_evidence_bench_check.json" if a.check else "roof_evidence_bench.json")
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
    w, h = api.grid_dims(ext, BIN)
    d_img = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    th = ctx.grid_picture_dev(d_xyz.data_ptr(), n, ext, d_img.data_ptr(), bin=BIN)
    has_switch = hasattr(ctx, "set_footprint_screen")
    d_plane = n_planes = ok = ok_default = None
    if has_switch:
        d_plane = torch.empty(n, dtype=torch.int32, device="cuda")
        ctx.segment_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), api.default_params(k=15))
        n_planes = len(ctx.planes_fetch())
        fit = ctx.plane_fit_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), n_planes)
        ok, ok_default = api.plane_quality(fit, max_rms_mm=a.max_rms_mm), api.plane_quality(fit)
    if a.footprints:
        d_keep = None
        if has_switch:
            _, _, outs = stage_row(ctx, d_xyz, n, d_plane, n_planes, ok, ext, th, 1)
            d_keep = outs["keep"]
        row = dict({"mode": "footprints_process", "label": a.label, "case": case, "points": n, "reps": a.reps, "pid": os.getpid(),
                    "library": os.path.relpath(api._lib.LIB_PATH, _package_root())}, **footprints_row(ctx, d_img, w, h, d_keep, a.reps))
        print(json.dumps(row), flush=True)
        doc = json.load(open(out_path)) if os.path.exists(out_path) else {"tool": "tests/tools/evidence_bench.py", "rows": []}
        doc["rows"].append(row)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
        ctx.close()
        return
    rows, good = [], True
    row, e, outs = stage_row(ctx, d_xyz, n, d_plane, n_planes, ok, ext, th, a.reps)
    row = dict({"mode": "stage", "case": case, "points": n, "sheet_points": n_sheet, "reps": a.reps, "planes": n_planes,
                "max_rms_mm": a.max_rms_mm, "planes_ok": int(ok.sum()), "planes_ok_at_100_mm": int(ok_default.sum()),
                "ground_th": float(th)}, **row)
    if a.check:
        cases = evidence_cases()
        plane = d_plane.cpu().numpy()
        want = cases.eref.evidence(xyz, plane, n_planes, ok, ext, BIN, th, cases.eref.params())
        diff = next((k for k in ("width", "height") + cases.eref.FIGURES if getattr(e, k) != getattr(want, k)), None)
        diff = diff or next((k for k in IMAGES if not np.array_equal(outs[k].cpu().numpy(), getattr(want, k))), None)
        row["equal_to_restatement"] = diff is None
        if diff is not None:
            row["first_difference"], good = diff, False
    rows.append(row)
    print(json.dumps(row), flush=True)
    d_keep = outs["keep"].clone()
    # beside the stage, on the same cloud
    d_map, b, _, _, _ = tbench.building_map(ctx, d_xyz, n, ext)
    d_bidx = torch.empty(n, dtype=torch.int32, device="cuda")
    _, assign_ms, _ = sbench.timed(lambda: ctx.assign_buildings_dev(d_xyz.data_ptr(), n, d_map.data_ptr(), b, d_bidx.data_ptr(), bin=BIN,
                                                                     ground_th=th), a.reps)
    copy_ms = sbench.copy_ms(12 * n, a.reps)
    beside = {"mode": "beside", "case": case, "points": n, "assign_buildings_dev_ms": sbench.stat(assign_ms),
              "copy_12_bytes_per_point_ms": sbench.stat(copy_ms),
              "roof_evidence_over_assign": round(row["roof_evidence_dev_ms"]["median"] / max(med(assign_ms), 1e-9), 3),
              "counts_pass_over_copy": round(row["ms_counts"]["median"] / max(med(copy_ms), 1e-9), 3)}
    del d_map, d_bidx
    rows.append(beside)
    print(json.dumps(beside), flush=True)
    for r in (0, 3, 15):
        rr, _, _ = stage_row(ctx, d_xyz, n, d_plane, n_planes, ok, ext, th, a.reps, r=r)
        rows.append({"mode": "radius", "case": case, "r": r, "width": w, "height": h, "ms_window": rr["ms_window"],
                     "ms_counts": rr["ms_counts"], "pixels_kept": rr["pixels_kept"]})
        print(json.dumps(rows[-1]), flush=True)
    order = np.argsort((xyz[:, 1] // BIN).astype(np.int64) * w + xyz[:, 0] // BIN, kind="stable")
    d_sxyz = torch.from_numpy(np.ascontiguousarray(xyz[order])).cuda()
    d_splane = torch.from_numpy(np.ascontiguousarray(d_plane.cpu().numpy()[order])).cuda()
    for name, dx, dp in (("shuffled", d_xyz, d_plane), ("sorted by pixel", d_sxyz, d_splane)):
        rr, ee, _ = stage_row(ctx, dx, n, dp, n_planes, ok, ext, th, a.reps)
        rows.append({"mode": "order", "case": case, "order": name, "ms_counts": rr["ms_counts"], "n_counted": ee.n_counted,
                     "n_planar": ee.n_planar, "pixels_kept": ee.pixels_kept})
        print(json.dumps(rows[-1]), flush=True)
    del d_sxyz, d_splane
    rows.append(dict({"mode": "footprints", "case": case, "points": n, "reps": a.reps},
                     **footprints_row(ctx, d_img, w, h, d_keep, a.reps)))
    print(json.dumps(rows[-1]), flush=True)
    with open(out_path, "w") as f:
        json.dump({"tool": "tests/tools/evidence_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    ctx.close()
    if not good:
        sys.exit(1)


if __name__ == "__main__":
    main()
