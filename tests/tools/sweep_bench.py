#!/usr/bin/env python3
"""Times the clean outlines with the sweep detection off (mode 0) and repairing (mode 2; bs_set_outline_sweeps) on urban at
--points (bench.py's urban_50m at the default) at bin 100 and bin 25 and at tolerances of 1, 2 and 4 pixels, through the chain
of tests/tools/uncross_bench.py.  HIP events on the context's stream; the two modes alternate in the same run, call by call,
median of --reps after 2 warm-ups each, with min and max.  Per row: the clean count in either mode, ms_detect and ms_sweep,
the ratio mode 2 / mode 0, the sweep figures, and under both modes n_failed_labels of the outline triangles, the open
buildings of the polygon solids, and n_uncovered and n_multi of the model raster.
--check compares every array, total and sweep figure of mode 2 with the restatement tests/sweep_ref (the cloud capped at 5 M
points).
usage: python tests/tools/sweep_bench.py [--reps 7] [--points 50000000] [--check] [--out profiles/outline_sweeps_bench.json]"""
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
import polysolid_bench as pbench  # noqa: E402  (the chain up to the facet image)
import simplify_bench as sbench  # noqa: E402  (the statistics)
from buildingsegment_amd import api, synth  # noqa: E402

TOLERANCES_PX = (1, 2, 4)
FIGURES = ("n_lens_segments_first", "n_sweeping_first", "n_sweeping_only_first", "n_swept_pairs_first", "max_abs_winding",
           "sweep_rounds", "n_sweeping_left", "n_items_first", "n_items_swapped_first", "n_candidates_first", "n_exact_first",
           "n_exact_wave_first", "n_rejected_first")


def sweep_ref():
    spec = importlib.util.spec_from_file_location("sweep_ref", os.path.join(ROOT, "tests", "sweep_ref", "sweep_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["sweep_ref"] = mod
    spec.loader.exec_module(mod)
    return mod


def alternated(ctx, count, reps):
    """mode 0 and mode 2 call by call: per mode (the last result, its sweep figures, the ms of every timed call, the stage
    times of every timed call)"""
    out = {0: [None, None, [], []], 2: [None, None, [], []]}
    for it in range(reps + 2):
        for mode in (0, 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(sbench.STREAM)
            c = count(mode)
            b.record(sbench.STREAM)
            b.synchronize()
            s = ctx.outline_sweeps()
            out[mode][0], out[mode][1] = c, s
            if it >= 2:
                out[mode][2].append(a.elapsed_time(b))
                out[mode][3].append(dict(c.info, ms_sweep=s.ms_sweep))
    return out


def case(ctx, n, bin_, px, im, reps, check):
    d_facet, d_top, w, h, n_facets, facet_building, nb, base_z, _ = im
    num, den = api.simplify_tolerance(px * bin_, bin_)
    args = (d_facet.data_ptr(), d_top.data_ptr(), w, h, n_facets)
    d_lb = torch.from_numpy(facet_building if n_facets else np.zeros(1, np.int32)).cuda()
    torch.cuda.synchronize()
    res = alternated(ctx, lambda mode: ctx.clean_outlines_dev(*args, num, den, sweeps=mode)[0], reps)
    c0, c2, s2 = res[0][0], res[2][0], res[2][1]
    row = {"case": f"urban_{n}_bin{bin_}_tol{px}px", "points": n, "bin": bin_, "tolerance_px": px, "tol2": [num, den], "width": w,
           "height": h, "reps": reps, "facets": n_facets, "n_nodes": c0.n_nodes, "segments": c0.n_svertices_before,
           "n_marked_first": c0.n_marked_first}
    for mode in (0, 2):
        c = res[mode][0]
        row[f"mode{mode}"] = {"clean_outlines_count_dev_ms": sbench.stat(res[mode][2]),
                              "ms_detect": sbench.stat([x["ms_detect"] for x in res[mode][3]]),
                              "ms_repair": sbench.stat([x["ms_repair"] for x in res[mode][3]]),
                              "ms_sweep": sbench.stat([x["ms_sweep"] for x in res[mode][3]]),
                              "repair_rounds": c.repair_rounds, "n_forced": c.n_forced, "n_svertices": c.n_svertices}
        ctx.set_outline_sweeps(mode)
        try:
            p, t = ctx.poly_solids_dev(*args, d_lb.data_ptr(), nb, num, den, bin=bin_, base_z=base_z)[:2]
            r = ctx.model_raster_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h)
        finally:
            ctx.set_outline_sweeps(0)
        row[f"mode{mode}"].update(n_failed_labels=t.n_failed_labels, n_open_buildings=p.n_open_buildings,
                                  n_uncovered=r.n_uncovered, n_multi=r.n_multi)
    row["sweeps"] = {k: getattr(s2, k) for k in FIGURES}
    m0, m2 = (row[f"mode{m}"]["clean_outlines_count_dev_ms"]["median"] for m in (0, 2))
    row["mode2_over_mode0"] = round(m2 / m0, 3)
    row["ms_sweep_over_mode0_detect"] = round(row["mode2"]["ms_sweep"]["median"] / max(row["mode0"]["ms_detect"]["median"], 1e-9), 3)
    if check:
        wref = sweep_ref()
        lab, top = d_facet.cpu().numpy(), d_top.cpu().numpy()
        got = ctx.clean_outlines(lab, top, n_labels=n_facets, num=num, den=den, sweeps=2)[0]
        s = ctx.outline_sweeps()
        _, _, want = wref.clean(lab, top, n_facets, num, den, mode=2)
        diff = wref.same(got, want, wref.DEVICE_FIELDS)
        if diff is None:
            diff = next((f for f in wref.SWEEP_FIELDS if getattr(s, f) != getattr(want, f)), None)
        row["equal_to_restatement"] = diff is None
        if diff is not None:
            row["first_difference"] = diff
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = "outline_sweeps_bench_check.json" if a.check else "outline_sweeps_bench.json"
    out_path = a.out or os.path.join(ROOT, "profiles", name)
    ctx = api.Context(0)
    sbench.STREAM = torch.cuda.Stream()
    ctx.set_stream(sbench.STREAM.cuda_stream)
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
        im = pbench.facet_image(ctx, xyz, d_xyz, d_plane, planes, ext, bin_, 1)
        for px in TOLERANCES_PX:
            rows.append(case(ctx, n, bin_, px, im, a.reps, a.check))
        del im
        torch.cuda.empty_cache()
    out = {"tool": "tests/tools/sweep_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()
    if a.check and not all(r["equal_to_restatement"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
