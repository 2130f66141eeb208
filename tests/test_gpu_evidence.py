"""Roof evidence on the device (bs_roof_evidence, bs_roof_evidence_dev; include/bs_api.h) against the numpy restatement
tests/evidence_ref, the footprint screen (bs_set_footprint_screen) in bs_footprints against tests/footprint_ref on the AND-ed
mask, and evidence= end to end on the boxes with trees.  Everything is an exact integer: every comparison is ==."""
import ctypes as C

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_evidence_cpu import BY_NAME, brute, cases, eref, gref, premise, ref  # noqa: E402

pytestmark = pytest.mark.gpu
PATTERN = -0x5A5A5A5B
IMAGES = eref.IMAGES
SCALARS = ("width", "height") + eref.FIGURES
LARGE = {c["name"]: c for c in cases.large()}
_LARGE_REF = {}


def large_ref(name):
    if name not in _LARGE_REF:
        _LARGE_REF[name] = eref.evidence(*cases.args(LARGE[name]))
    return _LARGE_REF[name]


def run(ctx, c, **kw):
    """the host entry point on a case, under the case's ground model"""
    ctx.set_ground_model(*(c["model"] if c["model"] is not None else (None,)))
    try:
        return ctx.roof_evidence(c["xyz"], c["plane_idx"], c["n_planes"], c["plane_ok"], c["extent"], c["bin"], c["ground_th"],
                                 c["params"], **kw)
    finally:
        ctx.set_ground_model(None)


def differs(got, want, images=IMAGES):
    """None if the device's RoofEvidence equals the restatement's result everywhere, else the first name that differs"""
    for k in SCALARS:
        if getattr(got, k) != getattr(want, k):
            return k, getattr(got, k), getattr(want, k)
    for k in images:
        a, b = getattr(got, k), getattr(want, k)
        if a.dtype != b.dtype or not np.array_equal(a, b):
            return k
    return None


def on_device(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("name", [c["name"] for c in cases.CASES])
def test_case(gpu_ctx, name):
    """every small case through the host entry point: keep, the four images and every figure"""
    c = BY_NAME[name]
    got, want = run(gpu_ctx, c), ref(name)
    assert differs(got, want) is None, (name, differs(got, want))
    p = c["params"]
    assert (got.r, got.min_points, got.num, got.den) == (p["r"], p["min_points"], p["num"], p["den"])
    assert got.n_points == len(c["xyz"]) and (got.grid, got.tile) == (_lib.GROUND_GRID, _lib.EVIDENCE_TILE)


@pytest.mark.parametrize("name", list(LARGE))
def test_large_case(gpu_ctx, name):
    """one more and one less than the LDS tile, 3 x 700 and 700 x 3, windows over four tiles, more tiles than one sweep of the
    window kernel's grid, more points than one sweep of the counts pass, and the ground model on a larger lattice"""
    got, want = run(gpu_ctx, LARGE[name]), large_ref(name)
    assert differs(got, want) is None, (name, differs(got, want))
    if name == "sweep_points":  # thousands of adds on one pixel
        assert got.above.max() > 1000 and got.n_points > 256 * got.grid
    if name == "sweep_pixels":
        assert -(-got.width // got.tile) * -(-got.height // got.tile) > _lib.EVIDENCE_GRID
    figures_only = run(gpu_ctx, LARGE[name], images=False)
    assert figures_only.above is None and differs(figures_only, want, ("keep",)) is None


def test_cases_on_the_device(gpu_ctx):
    """what the hand-made cases are for, read from the device's result"""
    a = run(gpu_ctx, BY_NAME["share_boundary"])
    (xk, yk), (xd, yd) = cases.BOUNDARY_KEPT, cases.BOUNDARY_DROPPED
    assert (a.win_above[yk, xk], a.win_planar[yk, xk], a.keep[yk, xk]) == (4, 2, 1)
    assert (a.win_above[yd, xd], a.win_planar[yd, xd], a.keep[yd, xd]) == (5, 2, 0)
    x, y = cases.THIN_AT
    a, b = run(gpu_ctx, BY_NAME["min_points_at"]), run(gpu_ctx, BY_NAME["min_points_over"])
    assert (a.keep[y, x], a.pixels_kept, a.pixels_thin) == (1, 9, 0) and (b.keep[y, x], b.pixels_kept, b.pixels_thin) == (0, 0, 9)
    a = run(gpu_ctx, BY_NAME["all_below"])
    assert not a.keep.any() and (a.n_counted, a.max_window) == (0, 0)
    a = run(gpu_ctx, BY_NAME["labels"])
    assert (a.n_counted, a.n_planar) == (5, 1) and a.keep[1].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    # the model decides: without it the same call gives another image
    c = BY_NAME["model"]
    assert differs(run(gpu_ctx, dict(c, model=None)), ref("model")) is not None


def test_null_outputs_and_errors(gpu_ctx):
    """the device entry point: each optional image NULL in turn, and every error of the definition: the outputs and the struct
    are untouched -- also by a point outside the lattice, which only the device finds -- and the context stays usable"""
    import torch
    ctx = gpu_ctx
    c, want = LARGE["tile_plus"], large_ref("tile_plus")
    w, h, n = want.width, want.height, len(c["xyz"])
    d_xyz, d_lab = on_device(c["xyz"], c["plane_idx"])
    outs = [torch.full((h, w), 0xA5, dtype=torch.uint8, device="cuda")]
    outs += [torch.full((h, w), PATTERN, dtype=torch.int32, device="cuda") for _ in range(4)]
    fills = [0xA5] + [PATTERN] * 4
    ptrs = [o.data_ptr() for o in outs]
    ext = np.ascontiguousarray(c["extent"], np.int32)
    ok = np.ascontiguousarray(c["plane_ok"], np.uint8)
    p = c["params"]

    def stage(out, xyz=d_xyz.data_ptr(), n=n, lab=d_lab.data_ptr(), n_planes=c["n_planes"], extent=ext, bin=c["bin"], params=p,
              outputs=ptrs):
        return ctx._L.bs_roof_evidence_dev(ctx._h, xyz, n, lab, n_planes, ok.ctypes.data, extent.ctypes.data if extent is not None
                                           else None, bin, c["ground_th"], params["r"], params["min_points"], params["num"],
                                           params["den"], *outputs, out)

    def untouched(**kw):
        out = _lib.RoofEvidence()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        rc = stage(C.byref(out), **kw)
        msg = ctx._L.bs_last_error(ctx._h)
        torch.cuda.synchronize()
        assert bytes(out) == b"\x5a" * C.sizeof(out) and all(bool((o == f).all()) for o, f in zip(outs, fills)), kw
        return rc, msg

    def moved(col, v):
        x = c["xyz"].copy()
        x[n // 2, col] = v
        return on_device(x)[0]

    assert stage(None) == -1
    invalid = [dict(xyz=None), dict(lab=None), dict(extent=None), dict(n=0), dict(bin=0), dict(n_planes=-1),
               dict(extent=np.array([-1, 5, 0], np.int32)), dict(outputs=[None] + ptrs[1:])]
    invalid += [dict(params=dict(p, **kw)) for kw in (dict(r=-1), dict(r=16), dict(min_points=0), dict(den=0), dict(num=-1),
                                                      dict(num=3, den=2))]
    for kw in invalid:
        assert untouched(**kw)[0] == -1, kw
    rc, msg = untouched(n=1 << 29)
    assert rc == -2 and b"2^29" in msg
    rc, msg = untouched(extent=np.array([2 ** 31 - 1, 2 ** 31 - 1, 0], np.int32), bin=1)
    assert rc == -2 and b"pixels" in msg
    for col, v in ((0, -1), (1, -1), (0, w * c["bin"]), (1, h * c["bin"])):
        bad = moved(col, v)
        rc, msg = untouched(xyz=bad.data_ptr())
        assert rc == -2 and b"outside the lattice" in msg, (col, v, msg)
    inside = moved(0, w * c["bin"] - 1)  # the last pixel of a row
    out = _lib.RoofEvidence()
    assert stage(C.byref(out), xyz=inside.data_ptr()) == 0 and out.n_points == n
    # each optional image NULL in turn, and all of them: the outputs given are written
    names = ("d_above", "d_planar", "d_win_above", "d_win_planar")
    for skip in (1, 2, 3, 4, (1, 2, 3, 4)):
        skip = (skip,) if isinstance(skip, int) else skip
        for o, f in zip(outs, fills):
            o.fill_(f)
        got = ctx.roof_evidence_dev(d_xyz.data_ptr(), n, d_lab.data_ptr(), c["n_planes"], ext, ptrs[0], ok, c["bin"], c["ground_th"],
                                    p, **{k: (0 if j + 1 in skip else q) for j, (k, q) in enumerate(zip(names, ptrs[1:]))})
        assert got.keep is None and differs(got, want, ()) is None, differs(got, want, ())
        for j, (o, f, field) in enumerate(zip(outs, fills, IMAGES)):
            a = o.cpu().numpy()
            assert np.array_equal(a, np.full(a.shape, f, a.dtype) if j in skip else getattr(want, field)), (skip, field)
    with pytest.raises(api.BsError):
        ctx.roof_evidence(c["xyz"], c["plane_idx"], c["n_planes"], ok, ext, c["bin"], c["ground_th"], dict(p, r=16))
    with pytest.raises(ValueError):
        ctx.roof_evidence(c["xyz"], c["plane_idx"], c["n_planes"], ok[:2], ext, c["bin"], c["ground_th"], p)
    assert differs(run(ctx, c), want) is None  # the context stays usable


# ---- the screen ---------------------------------------------------------------------------------------------------------------
def same_footprints(fp, mask, want, want_mask):
    assert np.array_equal(mask, want_mask * 255)
    assert len(fp.contours) == len(want.contours) and all(np.array_equal(a, b) for a, b in zip(fp.contours, want.contours))
    assert np.array_equal(fp.area, want.area) and np.array_equal(fp.perimeter, want.perimeter)


def footprint_bytes(fp, mask):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in [mask, fp.area, fp.perimeter] + list(fp.contours))


def test_screen_in_the_footprints(gpu_ctx):
    """with the switch on, the footprints are those of tests/footprint_ref on the AND-ed mask; off and cleared, every byte is
    that of the call before it was ever set; wrong dimensions and a batch of two tiles refuse; the _dev form reads the
    caller's buffer at every call"""
    import torch
    ctx = gpu_ctx
    rng = np.random.default_rng(5)
    h, w = 67, 131
    m = np.zeros((h, w), np.uint8)
    for _ in range(14):  # blobs, some of which touch
        y, x = int(rng.integers(0, h - 12)), int(rng.integers(0, w - 20))
        m[y:y + int(rng.integers(3, 12)), x:x + int(rng.integers(3, 20))] = 1
    img = np.zeros((h, w, 3))
    img[..., 1] = np.where(m, rng.uniform(1.0, 30.0, (h, w)), 0.0)  # some of the foreground is under the threshold
    keep = (rng.random((h, w)) < 0.8).astype(np.uint8)
    keep[:, 40:60] = 0
    assert ctx.footprint_screen() is None
    before = ctx.footprints(img, return_mask=True)
    plain, plain_mask = eref._fref().footprints(img)
    same_footprints(*before, plain, plain_mask)
    for kw in (dict(), dict(iterations=0), dict(threshold=100, kernel_size=3, iterations=1)):
        ctx.set_footprint_screen(keep)
        assert np.array_equal(ctx.footprint_screen(), keep)
        got = ctx.footprints(img, return_mask=True, **kw)
        want, want_mask = eref.screened_footprints(img, keep, **kw)
        same_footprints(*got, want, want_mask)
        ctx.set_footprint_screen(None)
    assert footprint_bytes(*got) != footprint_bytes(*before) and not want_mask[:, 42:58].any()
    assert ctx.footprint_screen() is None and footprint_bytes(*ctx.footprints(img, return_mask=True)) == footprint_bytes(*before)
    # an all-ones screen changes nothing; a RoofEvidence stands for its keep
    ctx.set_footprint_screen(np.ones((h, w), np.uint8))
    assert footprint_bytes(*ctx.footprints(img, return_mask=True)) == footprint_bytes(*before)
    # wrong dimensions, batches
    ctx.set_footprint_screen(keep[:, :-1])
    with pytest.raises(api.BsError, match="differ"):
        ctx.footprints(img)
    ctx.set_footprint_screen(keep[:-1])
    with pytest.raises(api.BsError, match="differ"):
        ctx.footprints(img)
    ctx.set_footprint_screen(keep)
    with pytest.raises(api.BsError, match="more than one tile"):
        ctx.footprints_batch([img, img])
    fps, masks = ctx.footprints_batch([img], return_mask=True)
    want, want_mask = eref.screened_footprints(img, keep)
    same_footprints(fps[0], masks[0], want, want_mask)
    # the device form keeps the caller's pointer: change the buffer between two calls
    d_keep, = on_device(keep)
    ctx.set_footprint_screen((d_keep.data_ptr(), w, h), device=True)
    same_footprints(*ctx.footprints(img, return_mask=True), want, want_mask)
    keep2 = keep.copy()
    keep2[:, 40:60] = 1
    keep2[20:30] = 0
    d_keep.copy_(torch.from_numpy(keep2))
    torch.cuda.synchronize()
    assert np.array_equal(ctx.footprint_screen(), keep2)
    same_footprints(*ctx.footprints(img, return_mask=True), *eref.screened_footprints(img, keep2))
    # a screen for one call restores the device pointer behind it
    with ctx._footprint_screen(keep):
        same_footprints(*ctx.footprints(img, return_mask=True), want, want_mask)
    same_footprints(*ctx.footprints(img, return_mask=True), *eref.screened_footprints(img, keep2))
    ctx.set_footprint_screen(None)
    assert footprint_bytes(*ctx.footprints(img, return_mask=True)) == footprint_bytes(*before)
    two = ctx.footprints_batch([img, img], return_mask=True)
    assert footprint_bytes(two[0][1], two[1][1]) == footprint_bytes(*before)
    for bad in (dict(width=0, height=4), dict(width=4, height=0)):
        assert ctx._L.bs_set_footprint_screen(ctx._h, keep.ctypes.data, bad["width"], bad["height"]) == -1
    assert ctx.footprint_screen() is None


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_end_to_end_buildings(gpu_ctx, oracle):
    """segment -> buildings(evidence={}) on the boxes with trees: the map is the CPU chain's, three buildings; without
    evidence= the tree is a building; the context's own screen survives the call"""
    ctx = gpu_ctx
    s = premise(oracle, 0)
    xyz = s.xyz
    _, _, plane_idx, planes = ctx.segment(xyz, api.default_params(k=15))
    assert len(planes) == s.n_planes and np.array_equal(plane_idx, s.labels)
    with pytest.raises(ValueError):
        ctx.buildings(xyz, evidence={})
    out = ctx.buildings(xyz, plane_idx, len(planes), evidence={})
    assert len(out) == 3 and ctx.footprint_screen() is None
    fp, b, ev = out
    assert differs(ev, s.screen.evidence, ("keep",)) is None and np.array_equal(ev.plane_ok, s.ok)
    scores = gref.box_scores(b.map, s.truth)
    print(f"level, evidence: buildings {b.n_buildings}, IoU {scores}, {ev.info}")
    assert b.n_buildings == 3 and np.array_equal(b.map, s.screen.buildings.map) and min(scores) >= 0.95
    fp0, b0 = ctx.buildings(xyz, plane_idx, len(planes))
    assert b0.n_buildings == s.plain.n_buildings > 3 and np.array_equal(b0.map, s.plain.map)
    assert (ev.n_planes, ev.planes_ok) == (s.n_planes, int(s.ok.sum()))
    # a rule that no plane passes: a warning, and an all-zero keep
    with pytest.warns(RuntimeWarning, match="none of the"):
        none = ctx._evidence(xyz, plane_idx, len(planes), cases.BIN, s.th, dict(max_rms_mm=0))
    assert none.planes_ok == 0 < none.n_planes and not none.keep.any() and none.n_planar == 0
    # the quality rule alone
    q = ctx.buildings(xyz, plane_idx, len(planes), evidence=dict(r=0))
    assert np.array_equal(q[1].map, s.quality.buildings.map)
    # a screen of the context's own survives the call, and is not the one the call used
    mine = np.ones_like(ev.keep)
    mine[:5] = 0
    ctx.set_footprint_screen(mine)
    try:
        assert np.array_equal(ctx.buildings(xyz, plane_idx, len(planes), evidence={})[1].map, b.map)
        assert np.array_equal(ctx.footprint_screen(), mine)
    finally:
        ctx.set_footprint_screen(None)


def test_end_to_end_solids(gpu_ctx, oracle):
    """segment -> solid_model(evidence={}, ground={}) on the slope with trees: as many solids as boxes, the Ground and the
    RoofEvidence returned last in this order, both switches restored"""
    ctx = gpu_ctx
    s = premise(oracle, 100)
    xyz = s.xyz
    _, _, plane_idx, planes = ctx.segment(xyz, api.default_params(k=15))
    assert np.array_equal(plane_idx, s.labels)
    out = ctx.solid_model(xyz, plane_idx, planes, refit=True, evidence={}, ground={})
    assert len(out) == 6 and ctx.footprint_screen() is None and ctx.ground_model() is None
    fp, b, roofs, sol, g, ev = out
    assert isinstance(g, api.Ground) and isinstance(ev, api.RoofEvidence)
    print("slope 100 with trees:", b.n_buildings, sol.pixels.tolist(), gref.box_scores(b.map, s.truth))
    assert b.n_buildings == 3 == sol.n_buildings and (sol.pixels > 0).all() and min(gref.box_scores(b.map, s.truth)) >= 0.95
    assert np.array_equal(b.map, s.screen.buildings.map) and differs(ev, s.screen.evidence, ("keep",)) is None
    plain = ctx.solid_model(xyz, plane_idx, planes, refit=True, ground={})
    assert len(plain) == 5 and plain[3].n_buildings == s.plain.n_buildings > 3
    out4 = ctx.roof_model(xyz, plane_idx, planes, refit=True, evidence={}, ground={})
    assert len(out4) == 5 and np.array_equal(out4[1].map, b.map) and isinstance(out4[3], api.Ground)
    out3 = ctx.buildings(xyz, plane_idx, len(planes), evidence={}, ground={})
    assert len(out3) == 4 and np.array_equal(out3[1].map, b.map) and isinstance(out3[3], api.RoofEvidence)
    assert len(ctx.solid_model(xyz, plane_idx, planes, refit=True)) == 4  # evidence=None returns what it returned before
