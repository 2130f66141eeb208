#!/usr/bin/env python3
"""Times the clean outlines (bs_clean_outlines_count_dev: the simplified count, the detections, the repair rounds, the
rings) on urban at --points (bench.py's urban_50m at the default) at bin 100 and bin 25, at tolerances of 1, 2 and 4 pixels
and at several broad-phase cell sizes, through the chain of tests/tools/simplify_bench.py in the same run.  HIP events on
the context's stream, median of --reps after 2 warm-ups, with min and max.  Beside them, re-measured in the same run on the
same image and at the same tolerance: bs_simple_outlines_count_dev, the yardstick.  Per row: n_marked_first,
repair_rounds, n_forced, entries per segment, max_cell_entries, the times of detect and repair, and the ratio of the whole
call to the simplified count alone.
--check compares every array and figure with the restatement tests/uncross_ref (the cloud capped at 5 M points).
usage: python tests/tools/uncross_bench.py [--reps 7] [--points 50000000] [--check] [--out profiles/outline_uncross_bench.json]"""
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
import simplify_bench as sbench  # noqa: E402  (the chain, the timer and the statistics)
from buildingsegment_amd import api, synth  # noqa: E402

STAGES = ("ms_simplify", "ms_detect", "ms_repair", "ms_rings")
TOLERANCES_PX = (1, 2, 4)
CELL_LOG2 = (2, 3, 4, 5, 6)


def uncross_ref():
    spec = importlib.util.spec_from_file_location("uncross_ref", os.path.join(ROOT, "tests", "uncross_ref", "uncross_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["uncross_ref"] = mod
    spec.loader.exec_module(mod)
    return mod


def cell_case(ctx, n, bin_, px, k, d_facet, d_top, w, h, n_facets, simple_ms, reps, want):
    num, den = api.simplify_tolerance(px * bin_, bin_)
    count = lambda: ctx.clean_outlines_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h, n_facets, num, den, -1, k)  # noqa: E731
    (c, s, plain), whole, runs = sbench.timed(count, reps)
    row = {"case": f"urban_{n}_bin{bin_}_tol{px}px_cell{k}", "points": n, "bin": bin_, "tolerance_px": px, "tol2": [num, den],
           "cell_log2": k, "width": w, "height": h, "reps": reps, "facets": n_facets, "n_rings": plain.n_rings,
           "n_nodes": c.n_nodes, "segments": c.n_svertices_before, "n_marked_first": c.n_marked_first,
           "repair_rounds": c.repair_rounds, "n_forced": c.n_forced, "n_marked_left": c.n_marked_left, "n_entries": c.n_entries,
           "entries_per_segment": round(c.n_entries / max(c.n_svertices_before, 1), 3), "max_cell_entries": c.max_cell_entries,
           "clean_outlines_count_dev_ms": sbench.stat(whole), "simple_outlines_count_dev_ms": sbench.stat(simple_ms)}
    for key in STAGES:
        row[key] = sbench.stat([x[0].info[key] for x in runs])
    row["clean_over_simple_count"] = round(row["clean_outlines_count_dev_ms"]["median"] /
                                           row["simple_outlines_count_dev_ms"]["median"], 3)
    if want is not None:
        uref = uncross_ref()
        nv = c.n_svertices
        d_xy = torch.empty((nv, 2), dtype=torch.int32, device="cuda")
        d_z, d_right = (torch.empty((nv,), dtype=torch.int32, device="cuda") for _ in range(2))
        d_flag = torch.empty((nv,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.clean_outlines_emit_dev(d_xy.data_ptr(), d_z.data_ptr(), d_right.data_ptr(), d_flag.data_ptr())
        c.sxy, c.sz, c.s_right, c.s_flag = (t.cpu().numpy() for t in (d_xy, d_z, d_right, d_flag))
        _, _, w_ = want(k)
        diff = uref.same(c, w_, uref.DEVICE_FIELDS)
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
    name = "outline_uncross_bench_check.json" if a.check else "outline_uncross_bench.json"
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
        d_facet, d_top, w, h, n_facets = sbench.facet_image(ctx, xyz, d_xyz, d_plane, planes, ext, bin_)
        for px in TOLERANCES_PX:
            num, den = api.simplify_tolerance(px * bin_, bin_)
            _, simple_ms, _ = sbench.timed(
                lambda: ctx.simplified_outlines_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h, n_facets, num, den), a.reps)
            want = None
            if a.check:
                lab, top = d_facet.cpu().numpy(), d_top.cpu().numpy()
                want = lambda k: uncross_ref().clean(lab, top, n_facets, num, den, cell_log2=k)  # noqa: E731
            for k in ((4, 1) if a.check else CELL_LOG2):
                rows.append(cell_case(ctx, n, bin_, px, k, d_facet, d_top, w, h, n_facets, simple_ms, a.reps, want))
        del d_facet, d_top
        torch.cuda.empty_cache()
    out = {"tool": "tests/tools/uncross_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
