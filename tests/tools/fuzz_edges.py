#!/usr/bin/env python3
"""Seeded inputs of the O(N) edge kernels (tests/edge_ref/cases.py: PLY ingest, the origin shift, tile boxes and the tile shift,
labels from owners, the row remap, the union-find hook), sizes and layouts drawn around every tile, wave and threshold.

On the CPU: every case is built and restated (tests/edge_ref/edge_ref.py), and the sizes reached are printed.  With --gpu
(MI355X box): the device entry point against the restatement, every comparison ==.  tests/test_gpu_edge_kernels.py runs the
first 40 seeds of every entry point through run() in its own process.
usage: python tests/tools/fuzz_edges.py [--cases 40] [--seed 0] [--entries ingest,shift,...] [--gpu]
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def load_edge_cases():
    if "edge_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("edge_cases", os.path.join(ROOT, "tests", "edge_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["edge_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["edge_cases"]


cases = load_edge_cases()
ref = cases.ref


# ---- the device calls (shared with tests/test_gpu_edge_kernels.py) -----------------------------------------------------------
def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()
    torch.cuda.synchronize()
    return t


def dev_ingest(ctx, records, n, stride, off, is_f64, scale, shift, lead=0):
    """(xyz, min) of bs_ingest_dev on records uploaded `lead` bytes behind the start of an allocation"""
    import torch
    body = to_dev(np.concatenate([np.full(lead, 0xA5, np.uint8), np.frombuffer(bytes(records), np.uint8)]))
    d_xyz = torch.full((n, 3), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mn = ctx.ingest_dev(body.data_ptr() + lead, n, stride, off, is_f64, d_xyz.data_ptr(), scale=scale, shift_to_origin=shift)
    return d_xyz.cpu().numpy(), mn


def want_ingest(records, n, stride, off, is_f64, scale, shift):
    xyz, bad = ref.ingest(records, n, stride, off, is_f64, scale)
    assert not bad
    if shift:
        return ref.shift(xyz)
    return xyz.astype(np.int64), np.zeros(3, np.int64)


def dev_shift(ctx, xyz):
    d = to_dev(xyz)
    mn = ctx.shift_to_origin_dev(d.data_ptr(), len(xyz))
    return d.cpu().numpy(), mn


def dev_tiles(ctx, xyz, off):
    """(boxes, minima, shifted points, boxes after the shift)"""
    d = to_dev(xyz)
    box = ctx.tile_boxes_dev(d.data_ptr(), off)
    mn = ctx.shift_tiles_to_origin_dev(d.data_ptr(), off)
    return box, mn, d.cpu().numpy(), ctx.tile_boxes_dev(d.data_ptr(), off)


def dev_labels(ctx, owner, seeds):
    import torch
    d_o, d_s = to_dev(owner), to_dev(seeds)
    d_l = torch.full((len(owner),), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.labels_from_owner_dev(d_o.data_ptr() if len(owner) else 0, len(owner), d_s.data_ptr() if len(seeds) else 0, len(seeds),
                              d_l.data_ptr() if len(owner) else 0)
    ctx.sync()
    return d_l.cpu().numpy()


def dev_remap(ctx, d_rows, n_rows, k, d_sg, n, bsearch):
    """(out, n_missing) through the binary search (bsearch) or the path the library chooses"""
    import torch
    d_out = torch.full((n_rows * k,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    os.environ.pop("BS_REMAP_BSEARCH", None)
    if bsearch:
        os.environ["BS_REMAP_BSEARCH"] = "1"
    try:
        miss = ctx.remap_rows_dev(d_rows.data_ptr(), n_rows, k, d_sg.data_ptr(), n, d_out.data_ptr())
    finally:
        os.environ.pop("BS_REMAP_BSEARCH", None)
    return d_out.cpu().numpy(), miss


def dev_hook(ctx, n_total, k, d_gidx, d_rows, d_parent):
    return ctx.cc_hook_dev(d_rows.data_ptr(), d_gidx.data_ptr(), int(d_gidx.shape[0]), k, d_parent.data_ptr(), n_total)


def dev_components(ctx, n_total, k, gidx, rows, max_calls=8):
    """(parent, hooks of every call) of one rank that calls until a call hooks nothing"""
    import torch
    d_g, d_r = to_dev(gidx), to_dev(rows)
    d_p = torch.arange(n_total, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hooks = []
    while len(hooks) < max_calls:
        hooks.append(dev_hook(ctx, n_total, k, d_g, d_r, d_p))
        if hooks[-1] == 0:
            break
    return d_p.cpu().numpy(), hooks


# ---- one case: the list of what differs (empty = equal) ----------------------------------------------------------------------
def same(name, got, want):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    if got.shape != want.shape:
        return [f"{name}: shape {got.shape} for {want.shape}"]
    d = np.flatnonzero((got != want).reshape(-1))
    return [f"{name}: {len(d)} of {got.size} differ, first at {int(d[0])}: {int(got.reshape(-1)[d[0]])} for {int(want.reshape(-1)[d[0]])}"] if len(d) else []


def check(entry, c, ctx):
    """restate case c of `entry`; with a context, run the device on it and return the differences"""
    if entry == "ingest":
        want, wmn = want_ingest(c["records"], c["n"], c["stride"], c["off"], c["is_f64"], c["scale"], c["shift"])
        if ctx is None:
            return []
        got, mn = dev_ingest(ctx, c["records"], c["n"], c["stride"], c["off"], c["is_f64"], c["scale"], c["shift"], c["lead"])
        return same("xyz", got, want) + same("min", mn, wmn)
    if entry == "shift":
        want, wmn = ref.shift(c["xyz"])
        if ctx is None:
            return []
        got, mn = dev_shift(ctx, c["xyz"])
        return same("xyz", got, want) + same("min", mn, wmn)
    if entry == "tiles":
        wbox, (wsh, wmn) = ref.tile_boxes(c["xyz"], c["off"]), ref.shift_tiles(c["xyz"], c["off"])
        if ctx is None:
            return []
        box, mn, sh, box2 = dev_tiles(ctx, c["xyz"], c["off"])
        return same("boxes", box, wbox) + same("minima", mn, wmn) + same("shifted", sh, wsh) + same("boxes after", box2, ref.tile_boxes(wsh, c["off"]))
    if entry == "labels":
        want = ref.labels_from_owner(c["owner"], c["seeds"])
        return [] if ctx is None else same("labels", dev_labels(ctx, c["owner"], c["seeds"]), want)
    if entry == "remap":
        want, wmiss = ref.remap(c["rows"], c["sg"])
        if ctx is None:
            return []
        got, miss = dev_remap(ctx, to_dev(c["rows"]), c["rows"].shape[0], c["rows"].shape[1], to_dev(c["sg"]), len(c["sg"]), False)
        return same("out", got, want.reshape(-1)) + ([] if (miss != 0) == wmiss else [f"n_missing {miss} for missing = {wmiss}"])
    if entry == "hook":
        want = ref.components(c["n_total"], c["gidx"], c["rows"])
        if ctx is None:
            return []
        got, hooks = dev_components(ctx, c["n_total"], c["k"], c["gidx"], c["rows"])
        ncomp = int((want == np.arange(c["n_total"])).sum())
        bad = same("parent", got, want)
        if hooks[-1] != 0 or sum(hooks) != c["n_total"] - ncomp:
            bad.append(f"hooks {hooks} for {c['n_total']} nodes in {ncomp} components")
        return bad
    raise ValueError(entry)


def run(ctx, entries=cases.FUZZ_ENTRIES, n_cases=cases.FUZZ_CASES, first=0, verbose=True):
    """(runs, [(entry, seed, differences)]) over n_cases seeds of every entry point"""
    runs, bad = 0, []
    for e in entries:
        for s in range(first, first + n_cases):
            d = check(e, cases.fuzz_case(e, s), ctx)
            runs += 1
            if d:
                bad.append((e, s, d))
                if verbose:
                    print(f"DIFFERENT {e} seed {s}: {'; '.join(d)}", flush=True)
    return runs, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=cases.FUZZ_CASES)
    ap.add_argument("--seed", type=int, default=0, help="first seed (the suite runs 0 .. 39)")
    ap.add_argument("--entries", default=",".join(cases.FUZZ_ENTRIES))
    ap.add_argument("--gpu", action="store_true")
    a = ap.parse_args()
    ctx = None
    if a.gpu:
        import torch
        torch.zeros(1, device="cuda")
        from buildingsegment_amd import api
        ctx = api.Context(0)
    t0 = time.time()
    runs, bad = run(ctx, a.entries.split(","), a.cases, a.seed)
    if ctx is not None:
        ctx.close()
    print(f"{runs} runs {'on the device' if a.gpu else 'restated only'}, {len(bad)} different, {time.time() - t0:.1f} s")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
