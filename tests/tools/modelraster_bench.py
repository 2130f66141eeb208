#!/usr/bin/env python3
"""Times the model raster (bs_model_raster_dev: rows, spans, pixel items, figures) on urban at --points (bench.py's urban_50m
at the default) at bin 100 and bin 25, at tolerances of 1, 2 and 4 pixels, through the chain of tests/tools/polysolid_bench.py
in the same run.  HIP events on the context's stream, median of --reps after 2 warm-ups, with min and max.  The four
phases are the library's own event times and include what the host does between them: the reads of n_rows, n_items and the
result, and in ms_figures the copies into the caller's images (the call with all three images NULL is timed beside it).  Beside them,
measured in the same run on the same image: a device-to-device copy of the bytes the call touches, and bs_solids_count_dev on
the same map.  Per row the fidelity figures themselves: lost, gained and twice pixels over all buildings, RMSE and the largest
error in millimetres.
--check compares every image and figure with the restatement tests/modelraster_ref (the cloud capped at 5 M points).
usage: python tests/tools/modelraster_bench.py [--reps 7] [--points 50000000] [--check] [--out profiles/model_raster_bench.json]"""
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
import simplify_bench as sbench  # noqa: E402  (the timer and the statistics)
from buildingsegment_amd import api, synth  # noqa: E402

STAGES = ("ms_rows", "ms_spans", "ms_pixels", "ms_figures")
TOLERANCES_PX = (1, 2, 4)


def modelraster_ref():
    spec = importlib.util.spec_from_file_location("modelraster_ref", os.path.join(ROOT, "tests", "modelraster_ref", "modelraster_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["modelraster_ref"] = mod
    spec.loader.exec_module(mod)
    return mod


def case(ctx, n, bin_, px, im, reps, check):
    d_facet, d_top, w, h, n_facets, facet_building, nb, base_z, pixel = im
    num, den = api.simplify_tolerance(px * bin_, bin_)
    t = ctx.outline_triangles_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h, n_facets, num, den)[0]
    d_img = [torch.empty((h, w), dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    call = lambda: ctx.model_raster_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h, *[i.data_ptr() for i in d_img])  # noqa: E731
    r, whole, runs = sbench.timed(call, reps)
    _, figures_only, _ = sbench.timed(lambda: ctx.model_raster_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h), reps)
    # the label image, two words of top a pixel, the three scratch images written and read, the three copies, the triangles, the
    # row records and both sums, and per pixel item one record and two atomics
    nbytes = (4 + 8 + 3 * 8 + 3 * 8) * w * h + 12 * t.n_triangles + 12 * t.n_triangles + 24 * r.n_rows + 8 * r.n_rows + 8 * r.n_items
    f = api.model_fidelity_of(r, facet_building if n_facets else np.zeros(0, np.int32), nb)
    sq = sum((int(hi) << 32) + int(lo) for hi, lo in zip(r.sq_hi, r.sq_lo))
    row = {"case": f"urban_{n}_bin{bin_}_tol{px}px", "points": n, "bin": bin_, "tolerance_px": px, "tol2": [num, den], "width": w,
           "height": h, "reps": reps, "facets": n_facets, "buildings": nb, "n_triangles": t.n_triangles,
           "n_failed_labels": t.n_failed_labels, "n_rows": r.n_rows, "n_items": r.n_items, "n_empty_spans": r.n_empty_spans,
           "max_span": r.max_span, "pixels": r.total_pixels, "model_pixels": r.total_model_pixels, "kept": r.total_kept,
           "lost": int(f.lost.sum()), "gained": int(f.gained.sum()), "twice": int(f.twice.sum()), "n_uncovered": r.n_uncovered,
           "n_spill": r.n_spill, "n_moved": r.n_moved, "n_multi": r.n_multi,
           "rmse_mm": round((sq / 4 / max(r.total_err_pixels, 1)) ** 0.5, 3), "max_abs_mm": r.max_abs_e2_all / 2,
           "mean_abs_mm": round(r.total_sum_abs_e2 / 2 / max(r.total_err_pixels, 1), 3),
           "buildings_with_twice": int((f.twice > 0).sum()),
           "model_raster_dev_ms": sbench.stat(whole), "model_raster_dev_without_images_ms": sbench.stat(figures_only),
           "touched_bytes": nbytes, "copy_of_touched_bytes_ms": sbench.stat(sbench.copy_ms(nbytes, reps)),
           "solids_count_dev_ms": pixel["solids_count_dev_ms"]}
    for key in STAGES:
        row[key] = sbench.stat([x.info[key] for x in runs])
    if check:
        mref = modelraster_ref()
        gt, gc, _, _ = ctx.outline_triangles(d_facet.cpu().numpy(), d_top.cpu().numpy(), n_labels=n_facets, num=num, den=den)
        want = mref.model_raster(gc, gt, d_facet.cpu().numpy(), d_top.cpu().numpy(), n_facets)
        r.model, r.cover, r.mz2 = (i.cpu().numpy() for i in d_img)
        diff = mref.same(r, want)
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
    name = "model_raster_bench_check.json" if a.check else "model_raster_bench.json"
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
        im = pbench.facet_image(ctx, xyz, d_xyz, d_plane, planes, ext, bin_, a.reps)
        for px in TOLERANCES_PX:
            rows.append(case(ctx, n, bin_, px, im, a.reps, a.check))
        del im
        torch.cuda.empty_cache()
    out = {"tool": "tests/tools/modelraster_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()
    if a.check and not all(r["equal_to_restatement"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
