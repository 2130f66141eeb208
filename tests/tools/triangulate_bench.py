#!/usr/bin/env python3
"""Times the outline triangles (bs_outline_triangles_count_dev: the clean count, the prologue, the three label kernels) on
urban at --points (bench.py's urban_50m at the default) at bin 100 and bin 25, at tolerances of 1, 2 and 4 pixels, through
the chain of tests/tools/uncross_bench.py in the same run.  HIP events on the context's stream, median of --reps after 2
warm-ups, with min and max.  Beside them, re-measured in the same run on the same image and at the same tolerance:
bs_clean_outlines_count_dev, the yardstick, and a device-to-device copy of the bytes the stage itself touches (12 per clean
vertex read, 12 per triangle written).  Per row: the triangles, bridges and failed labels, the labels by kernel path, the
largest label's occurrences with the path it takes and that kernel's time (the bound of its work item's), triangles per
second of the stage's own time, and ear tests per triangle.
--check compares every array and total with the restatement tests/triangulate_ref (the cloud capped at 5 M points).
usage: python tests/tools/triangulate_bench.py [--reps 7] [--points 50000000] [--check] [--out profiles/outline_triangles_bench.json]"""
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

STAGES = ("ms_clean", "ms_prologue", "ms_wave", "ms_lds", "ms_global")
TOLERANCES_PX = (1, 2, 4)


def triangulate_ref():
    spec = importlib.util.spec_from_file_location("triangulate_ref", os.path.join(ROOT, "tests", "triangulate_ref", "triangulate_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["triangulate_ref"] = mod
    spec.loader.exec_module(mod)
    return mod


def case(ctx, n, bin_, px, d_facet, d_top, w, h, n_facets, reps, check):
    num, den = api.simplify_tolerance(px * bin_, bin_)
    args = (d_facet.data_ptr(), d_top.data_ptr(), w, h, n_facets, num, den)
    _, clean_ms, _ = sbench.timed(lambda: ctx.clean_outlines_dev(*args), reps)
    (t, c, s, plain), whole, runs = sbench.timed(lambda: ctx.outline_triangles_dev(*args), reps)
    own = [sum(x[0].info[k] for k in STAGES[1:]) for x in runs]
    path = "wave" if t.max_label_occurrences <= t.wave_cap else "lds" if t.max_label_occurrences <= t.lds_cap else "global"
    nbytes = 12 * t.n_svertices + 12 * t.n_triangles
    row = {"case": f"urban_{n}_bin{bin_}_tol{px}px", "points": n, "bin": bin_, "tolerance_px": px, "tol2": [num, den], "width": w,
           "height": h, "reps": reps, "facets": n_facets, "n_rings": t.n_rings, "n_svertices": t.n_svertices,
           "n_triangles": t.n_triangles, "n_bridges": t.n_bridges, "n_failed_labels": t.n_failed_labels, "n_tests": t.n_tests,
           "tests_per_triangle": round(t.n_tests / max(t.n_triangles, 1), 3),
           "labels_by_path": [t.n_labels_wave, t.n_labels_lds, t.n_labels_global],
           "max_label_occurrences": t.max_label_occurrences, "largest_label_path": path,
           "outline_triangles_count_dev_ms": sbench.stat(whole), "clean_outlines_count_dev_ms": sbench.stat(clean_ms),
           "own_ms": sbench.stat(own), "touched_bytes": nbytes, "copy_of_touched_bytes_ms": sbench.stat(sbench.copy_ms(nbytes, reps))}
    for key in STAGES:
        row[key] = sbench.stat([x[0].info[key] for x in runs])
    row["largest_label_kernel_ms"] = row["ms_" + path]
    row["triangles_over_clean_count"] = round(row["outline_triangles_count_dev_ms"]["median"] /
                                              row["clean_outlines_count_dev_ms"]["median"], 3)
    row["triangles_per_second_of_own_time"] = round(t.n_triangles / max(row["own_ms"]["median"], 1e-6) * 1e3)
    if check:
        tref = triangulate_ref()
        d_tri = torch.empty((t.n_triangles, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.outline_triangles_emit_dev(d_tri.data_ptr())
        t.tri = d_tri.cpu().numpy()
        wp, _, wc = tref.uref.clean(d_facet.cpu().numpy(), d_top.cpu().numpy(), n_facets, num, den)
        diff = tref.same(t, tref.triangulate(wp, wc))
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
    name = "outline_triangles_bench_check.json" if a.check else "outline_triangles_bench.json"
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
            rows.append(case(ctx, n, bin_, px, d_facet, d_top, w, h, n_facets, a.reps, a.check))
        del d_facet, d_top
        torch.cuda.empty_cache()
    out = {"tool": "tests/tools/triangulate_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()
    if a.check and not all(r["equal_to_restatement"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
