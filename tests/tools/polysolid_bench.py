#!/usr/bin/env python3
"""Times the polygon solids (bs_poly_solids_count_dev: the triangle count, the twins, the vertices, the count; and
bs_poly_solids_emit_dev) on urban at --points (bench.py's urban_50m at the default) at bin 100 and bin 25, at tolerances of 1, 2
and 4 pixels, through the chain of tests/tools/triangulate_bench.py in the same run.  HIP events on the context's stream,
median of --reps after 2 warm-ups, with min and max.  Beside them, re-measured in the same run on the same image and at the
same tolerance: bs_outline_triangles_count_dev alone, a device-to-device copy of the bytes the stage writes (the mesh), and
the face count and the time of bs_solids_count_dev on the same map -- the pixel-exact mesh this stage exists to beat.  Per
row: vertices, faces, indices, walls, crossing walls and open buildings.
--check compares every array and figure with the restatement tests/polysolid_ref (the cloud capped at 5 M points).
usage: python tests/tools/polysolid_bench.py [--reps 7] [--points 50000000] [--check] [--out profiles/poly_solids_bench.json]"""
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

STAGES = ("ms_triangles", "ms_twins", "ms_vertices", "ms_count")
TOLERANCES_PX = (1, 2, 4)


def polysolid_ref():
    spec = importlib.util.spec_from_file_location("polysolid_ref", os.path.join(ROOT, "tests", "polysolid_ref", "polysolid_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["polysolid_ref"] = mod
    spec.loader.exec_module(mod)
    return mod


def facet_image(ctx, xyz, d_xyz, d_plane, planes, ext, bin_, reps):
    """the chain of simplify_bench.facet_image, which also keeps what this stage needs of it: the building of every facet,
    base_z, and the figures and the time of the pixel-exact solids on the same map"""
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
    solids, solids_ms, _ = sbench.timed(lambda: ctx.solids_dev(d_map.data_ptr(), d_roof.data_ptr(), w, h, normal, center, r.z_min,
                                                               r.z_max, bin_, base_z, flat, d_top=d_top.data_ptr()), reps)
    d_facet = torch.empty((h, w), dtype=torch.int32, device="cuda")
    f = ctx.roof_facets_dev(d_map.data_ptr(), d_roof.data_ptr(), d_top.data_ptr(), w, h, b.n_buildings, n_planes,
                            d_facet.data_ptr())
    torch.cuda.synchronize()
    pixel = {"n_vertices": solids.n_vertices, "n_faces": solids.n_faces, "n_indices": solids.n_indices,
             "solids_count_dev_ms": sbench.stat(solids_ms)}
    return d_facet, d_top, w, h, int(f.n_facets), np.ascontiguousarray(f.facet_building, np.int32), int(b.n_buildings), base_z, pixel


def case(ctx, n, bin_, px, im, reps, check):
    d_facet, d_top, w, h, n_facets, facet_building, nb, base_z, pixel = im
    num, den = api.simplify_tolerance(px * bin_, bin_)
    d_lb = torch.from_numpy(facet_building if n_facets else np.zeros(1, np.int32)).cuda()
    tri_args = (d_facet.data_ptr(), d_top.data_ptr(), w, h, n_facets, num, den)
    _, tri_ms, _ = sbench.timed(lambda: ctx.outline_triangles_dev(*tri_args), reps)
    count = lambda: ctx.poly_solids_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h, n_facets, d_lb.data_ptr(), nb, num, den,  # noqa: E731
                                        bin=bin_, base_z=base_z)
    (p, t, c, s, plain), whole, runs = sbench.timed(count, reps)
    own = [sum(x[0].info[k] for k in STAGES[1:]) for x in runs]
    d_vertex = torch.empty((p.n_vertices, 4), dtype=torch.int32, device="cuda")
    d_off = torch.empty((p.n_faces + 1,), dtype=torch.int32, device="cuda")
    d_idx = torch.empty((p.n_indices,), dtype=torch.int32, device="cuda")
    d_fb = torch.empty((p.n_faces,), dtype=torch.int32, device="cuda")
    d_kind = torch.empty((p.n_faces,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    emit = lambda: ctx.poly_solids_emit_dev(d_vertex.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), d_fb.data_ptr(),  # noqa: E731
                                            d_kind.data_ptr())
    _, emit_ms, _ = sbench.timed(emit, reps)
    nbytes = 16 * p.n_vertices + 4 * (p.n_faces + 1) + 4 * p.n_indices + 5 * p.n_faces
    row = {"case": f"urban_{n}_bin{bin_}_tol{px}px", "points": n, "bin": bin_, "tolerance_px": px, "tol2": [num, den], "width": w,
           "height": h, "reps": reps, "facets": n_facets, "buildings": nb, "base_z": base_z, "n_svertices": t.n_svertices,
           "n_triangles": t.n_triangles, "n_failed_labels": t.n_failed_labels, "n_vertices": p.n_vertices, "n_faces": p.n_faces,
           "n_indices": p.n_indices, "n_roof_faces": p.n_roof_faces, "n_wall_faces": p.n_wall_faces,
           "n_crossing_walls": p.n_crossing_walls, "n_open_buildings": p.n_open_buildings,
           "max_wall_vertices": p.max_wall_vertices_all, "total_volume6": p.total_volume6,
           "poly_solids_count_dev_ms": sbench.stat(whole), "outline_triangles_count_dev_ms": sbench.stat(tri_ms),
           "own_ms": sbench.stat(own), "poly_solids_emit_dev_ms": sbench.stat(emit_ms), "written_bytes": nbytes,
           "copy_of_written_bytes_ms": sbench.stat(sbench.copy_ms(nbytes, reps)), "pixel_solids": pixel,
           "faces_of_pixel_solids_per_face": round(pixel["n_faces"] / max(p.n_faces, 1), 1)}
    for key in STAGES:
        row[key] = sbench.stat([x[0].info[key] for x in runs])
    if check:
        pref = polysolid_ref()
        p.vertex, p.face_offset, p.face_index, p.face_building, p.face_kind = (x.cpu().numpy() for x in (d_vertex, d_off, d_idx, d_fb,
                                                                                                          d_kind))
        wp, _, wc = pref.uref.clean(d_facet.cpu().numpy(), d_top.cpu().numpy(), n_facets, num, den)
        want = pref.poly_solids(wp, wc, pref.tref.triangulate(wp, wc), facet_building, nb, bin_, base_z)
        diff = pref.same(p, want)
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
    name = "poly_solids_bench_check.json" if a.check else "poly_solids_bench.json"
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
        im = facet_image(ctx, xyz, d_xyz, d_plane, planes, ext, bin_, a.reps)
        for px in TOLERANCES_PX:
            rows.append(case(ctx, n, bin_, px, im, a.reps, a.check))
        del im
        torch.cuda.empty_cache()
    out = {"tool": "tests/tools/polysolid_bench.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()
    if a.check and not all(r["equal_to_restatement"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
