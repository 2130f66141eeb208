#!/usr/bin/env python3
"""Differential fuzzing of stages 4-6 (raster, footprints, buildings) against their CPU references (GPU box only).

Two kinds of case come from one seed.  A cloud case runs the whole chain on one random cloud: bs_grid_picture against
oracle.grid_picture, bs_footprints against tests/footprint_ref, bs_building_map / bs_assign_buildings /
bs_plane_buildings against tests/building_ref.  The device output of a stage is the input of the next stage on the
device AND in the reference, so a mismatch names its stage.  An image case feeds a synthetic f64 image (integer
boundaries of the quantisation, a far unique maximum, negative / NaN / inf / subnormal pixels) to bs_footprints and
bs_building_map.  Every comparison is ==.  --batch packs runs of consecutive cases as the tiles of
bs_grid_picture_batch / bs_footprints_batch and compares every tile with the reference and with its solo result.

Generation needs no device (tests/test_fuzz_stages_cpu.py uses it): make_case, draw_params, replay_case, coverage.
The main stream of a seed gives one sub-seed per case and everything of a case is drawn from that sub-seed, so
--only keeps the stream in step and no case is ever skipped.
usage: python tests/tools/fuzz_stages.py [--cases N] [--seed S] [--only I] [--batch] [--repeat R] [--log FILE] [--dump DIR]
With --batch, --only I runs the batch that holds case I and --repeat R repeats each batch call.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "footprint_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "building_ref"))

# the run of tests/test_gpu_fuzz_stages.py; tests/test_fuzz_stages_cpu.py asserts what these cases reach
GPU_TEST_SEED, GPU_TEST_CASES = 22, 44

I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
ZH_LDS = 4096                 # bs_raster.hip: height bins counted in LDS
FIG_CAP = 256                 # bs_building.hip: buildings whose figures are reduced in LDS
VOTE_LDS_CELLS = 8192         # bs_building.hip: vote table in LDS
VOTE_DENSE_CELLS = 1 << 22    # bs_building.hip: dense vote table in HBM; above: sorted keys
MAX_VOTE_CELLS = 2 * 10**7    # (the reference's dense count matrix stays below 200 MB)
MAX_PIXELS = 1_500_000        # raster of a cloud case
MAX_IMAGE = (3000, 4100)
MAX_CLOSE_WORK = 8e8          # pixels * kernel cells * passes of the sequential closing restatement (about 2 s)
MAX_BINS = 8_000_000
LARGE_IMAGE = 2048 * 256      # pixels; a size class, not a boundary of any code path: the coverage asks for one image above
                              # it, so that the per-tile maximum is the atomicMax of well over a hundred blocks

CLOUD_KINDS = ("boxes", "rings", "blob", "column", "pixel", "tower", "clusters", "urban", "sparse", "tiny")
IMAGE_KINDS = ("smooth", "spikes", "jrows", "unique_max", "equal", "zero")
SPECIALS = (-1.0, -0.0, float("nan"), float("-inf"), 5e-324, 2.0e-308, -1e300, -5e-324)


# ---- generation (no device) --------------------------------------------------------------------------------------

def _sheet(x0, x1, y0, y1, z, spacing):
    x, y = np.meshgrid(np.arange(x0, x1 + 1, spacing, dtype=np.int64), np.arange(y0, y1 + 1, spacing, dtype=np.int64),
                       indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, z, np.int64)], 1)


def _log_int(rng, lo, hi):
    return int(round(np.exp(rng.uniform(np.log(lo), np.log(hi)))))


def _cloud(rng):
    from buildingsegment_amd import synth
    draw = CLOUD_KINDS + ("tower", "sparse")  # (the two kinds whose regimes nothing else reaches: twice as likely)
    kind = draw[int(rng.integers(0, len(draw)))]
    if kind == "boxes":  # box buildings on a sparse ground sheet
        lo = int(rng.integers(8, 40))
        box = synth.boxes(n_boxes=int(rng.integers(1, 7)), seed=int(rng.integers(1, 10**6)), edge_lo=lo,
                          edge_hi=lo + int(rng.integers(1, 30)), pitch=int(rng.integers(3000, 9000)),
                          shuffle=False).astype(np.int64)
        m = int(rng.integers(0, 4000))
        mn, mx = box.min(0), box.max(0)
        pts = np.concatenate([box, _sheet(mn[0] - m, mx[0] + m, mn[1] - m, mx[1] + m, 0, int(rng.integers(150, 500)))])
    elif kind == "rings":  # ring roofs around courtyards whose floor is the sparse ground sheet
        parts, x0 = [], 0
        for _ in range(int(rng.integers(1, 5))):
            side, sp = int(rng.integers(6000, 20000)), int(rng.integers(40, 120))
            roof = _sheet(x0, x0 + side, 0, side, int(rng.integers(3000, 12000)), sp)
            t = int(side * rng.uniform(0.15, 0.35))
            inner = ((roof[:, 0] > x0 + t) & (roof[:, 0] < x0 + side - t) & (roof[:, 1] > t) & (roof[:, 1] < side - t))
            parts.append(roof[~inner])
            x0 += side + int(rng.integers(1500, 6000))
        every = np.concatenate(parts)
        mn, mx = every.min(0), every.max(0)
        pts = np.concatenate([every, _sheet(mn[0] - 2000, mx[0] + 2000, mn[1] - 2000, mx[1] + 2000, 0,
                                            int(rng.integers(250, 700)))])
        pts[:, :2] += rng.integers(-10, 11, (len(pts), 2))
    elif kind == "blob":
        n = _log_int(rng, 2, 300_000)
        L = max(int(50 * n ** (1 / 3) * rng.uniform(0.5, 6)), 2)
        pts = rng.integers(0, L, (n, 3))
    elif kind == "column":  # one (x, y), many heights
        n = _log_int(rng, 1, 5000)
        pts = np.stack([np.full(n, 5), np.full(n, 9), rng.integers(0, int(rng.choice([50, 30000, 3_000_000])), n)], 1)
    elif kind == "pixel":  # everything inside one pixel of most bins
        n = _log_int(rng, 1, 20000)
        pts = np.concatenate([rng.integers(0, int(rng.choice([1, 7, 30])), (n, 2)), rng.integers(0, 9000, (n, 1))], 1)
    elif kind == "tower":  # height bins far beyond the LDS histogram
        n = _log_int(rng, 100, 60000)
        top = int(rng.uniform(1e6, 6e6))
        z = rng.integers(0, top, n)
        if rng.random() < 0.6:  # most points high up: the ground threshold lies in a bin >= 4096 as well
            z = top - (top - z) // int(rng.integers(2, 50))
        pts = np.concatenate([rng.integers(0, int(rng.integers(100, 4000)), (n, 2)), z[:, None]], 1)
    elif kind == "clusters":
        n = _log_int(rng, 200, 100_000)
        c = rng.integers(0, 150_000, (int(rng.integers(2, 7)), 3))
        c[:, 2] //= 10
        pts = c[rng.integers(0, len(c), n)] + rng.integers(-400, 400, (n, 3))
    elif kind == "urban":
        pts = synth.urban(_log_int(rng, 20_000, 200_000), seed=int(rng.integers(1, 10**6)), shuffle=False,
                          spacing=int(rng.choice([150, 250, 400])))
    elif kind == "sparse":  # isolated points: hundreds to thousands of one-pixel buildings
        n = _log_int(rng, 400, 4000)
        S = int(100 * np.sqrt(n) * rng.uniform(6, 14))
        pts = np.concatenate([rng.integers(0, S, (n, 2)), rng.integers(0, 20000, (n, 1))], 1)
    else:  # tiny: fewer points than a wave, or a wave and one more
        n = int(rng.choice([1, 2, 5, 31, 63, 64, 65, int(rng.integers(1, 70))]))
        pts = np.concatenate([rng.integers(0, int(rng.choice([3, 500, 20000])), (n, 2)), rng.integers(0, 5000, (n, 1))], 1)
    pts = np.asarray(pts, dtype=np.int64)
    pts -= pts.min(0, keepdims=True)
    return dict(kind="cloud", sub=kind, xyz=np.ascontiguousarray(pts.astype(np.int32)))


def _edge_len(rng, tile, lo, hi):
    """a length in [lo, hi] whose padded size (+ 2) is a multiple of `tile`, one less or one more"""
    k = int(rng.integers(max((lo + 3) // tile, 1), max((hi + 1) // tile, 1) + 1))
    return int(np.clip(k * tile - 2 + int(rng.integers(-1, 2)), lo, hi))


def _image(rng):
    kind = IMAGE_KINDS[int(rng.integers(0, len(IMAGE_KINDS)))]
    cls = rng.random()
    if cls < 0.15:
        h, w = int(rng.integers(1, 21)), int(rng.integers(1, 21))
    elif cls < 0.5:
        h, w = _edge_len(rng, 16, 1, 100), _edge_len(rng, 64, 1, 400)
    elif cls < 0.88:
        h, w = int(rng.integers(20, 400)), int(rng.integers(20, 600))
    else:  # larger than one pass of the grid-stride maximum (2048 blocks of 256)
        h, w = int(rng.integers(700, MAX_IMAGE[0] + 1)), int(rng.integers(760, MAX_IMAGE[1] + 1))
    npix = h * w
    mx = float(rng.choice([255.0, 1.0, 30.0, 27.43, rng.uniform(0.1, 1e4), 1e-300, 1e300, 3e-320]))
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        f = np.sin(xx / rng.uniform(3, 40) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(3, 40)) + rng.uniform(-0.5, 1)
        ch = np.maximum(f, 0) * mx
    elif kind == "spikes":
        ch = np.where(rng.random((h, w)) < rng.uniform(0.002, 0.2), rng.random((h, w)) * mx, 0.0)
    elif kind == "jrows":  # every max * j / 255 with both neighbours: 255 * (v / max) on and next to every integer
        x = mx * np.arange(256) / 255.0
        trip = np.stack([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)], 1).ravel()
        trip = np.clip(trip, 0.0, mx)
        ch = np.resize(trip, npix).reshape(h, w).copy()
        if npix > len(trip):  # noise after the first run of the rows
            tail = ch.ravel()[len(trip):]
            tail[rng.random(len(tail)) < 0.5] = 0.0
        ch.ravel()[int(rng.integers(0, npix))] = mx
    elif kind == "unique_max":  # one pixel above everything else, anywhere: first, last, random
        ch = rng.random((h, w)) * mx * rng.uniform(0.05, 0.98)
        ch[rng.random((h, w)) < 0.5] = 0.0
        at = int(rng.choice([0, npix - 1, int(rng.integers(0, npix))]))
        ch.ravel()[at] = mx
    elif kind == "equal":
        ch = np.full((h, w), mx)
    else:
        ch = np.zeros((h, w))
    ch = np.ascontiguousarray(ch, dtype=np.float64)
    special = rng.random() < 0.4
    if special:
        at = rng.integers(0, npix, int(rng.integers(1, 20)))
        ch.ravel()[at] = rng.choice(SPECIALS, len(at))
        if rng.random() < 0.25:  # +inf is the maximum: every quotient is 0 or NaN
            ch.ravel()[int(rng.integers(0, npix))] = np.inf
    return dict(kind="image", sub=kind + ("+special" if special else ""), ch1=ch)


def make_case(rng):
    """One case from a generator: dict(kind="cloud", sub, xyz int32 [n, 3] shifted to its origin, generated order) or
    dict(kind="image", sub, ch1 f64 [h][w])."""
    return _cloud(rng) if rng.random() < 0.6 else _image(rng)


def quantised(ch1):
    """save_image's 8-bit value of every pixel as ref_mask defines it (one numpy line per C line)."""
    with np.errstate(all="ignore"):
        finite_max = np.where(np.isnan(ch1), 0.0, ch1).max(initial=0.0)
        mx = max(0.0, float(finite_max))
        if mx == 0:
            return np.zeros(ch1.shape, np.int64)
        t = 255.0 * (1.0 * ch1 / mx)
        return np.where(t > 0, t, 0.0).astype(np.int64)


def _bound_closing(npix, ks, it):
    while it > 0 and npix * ks * ks * 2.0 * it > MAX_CLOSE_WORK:
        if ks > 3 and (it == 1 or ks * ks > 4 * it):
            ks -= 2
        else:
            it -= 1
    return ks, it


def _footprint_params(rng, npix, q=None):
    """threshold, kernel_size, iterations over their whole ranges; q: quantised values to aim the threshold at"""
    c = rng.random()
    if q is not None and c < 0.45:
        v = int(q.ravel()[int(rng.integers(0, q.size))])
        thr = int(np.clip(v - int(rng.integers(0, 2)), 0, 255))
    elif c < 0.75:
        thr = int(rng.choice([0, 1, 10, 10, 128, 254, 255]))
    elif c < 0.9:
        thr = int(rng.integers(200, 256))
    else:
        thr = int(rng.integers(0, 256))
    ks = int(rng.choice([1, 3, 5, 5, 7, 9, 11, 13, 15]))
    it = int(rng.choice([0, 1, 2, 2, 3, 5, 16, int(rng.integers(0, 17))]))
    ks, it = _bound_closing(npix, ks, it)
    return dict(threshold=thr, kernel_size=ks, iterations=it)


def draw_params(rng, case):
    """The parameters of a case, drawn after it from the same generator; always inside the documented domains."""
    if case["kind"] == "image":
        return _footprint_params(rng, case["ch1"].size, quantised(case["ch1"]))
    xyz = case["xyz"]
    n, mx = len(xyz), xyz.max(0).astype(np.int64)
    sparse = case["sub"] == "sparse"
    bins = [7, 37, 100, 100, 1000, "edge", "edge", "edge"] + ([1] if max(mx[0], mx[1]) < 1200 else [])
    b = (37, 100)[int(rng.integers(0, 2))] if sparse else bins[int(rng.integers(0, len(bins)))]
    if b == "edge":  # the padded width mx / bin + 4 on a 64-pixel tile edge, one less or one more
        d, b = int(rng.integers(-1, 2)), 100
        for k in rng.permutation(np.arange(1, 20)):
            want = 64 * int(k) + d - 4
            cand = int(mx[0]) // want if want > 0 else 0
            if cand >= 1 and int(mx[0]) // cand == want and (mx[0] // cand + 2) * (mx[1] // cand + 2) <= MAX_PIXELS:
                b = cand
                break
    while (mx[0] // b + 8) * (mx[1] // b + 8) > MAX_PIXELS:
        b *= 2
    bh = int(rng.choice([1, 7, 250, 1000, 1000, 5000]))
    ext = mx.copy()
    if rng.random() < 0.5:  # an extent larger than the cloud, by a slack of its own per axis
        ext[:2] += rng.integers(0, 5 * b + 1, 2)
        ext[2] += int(rng.integers(0, 4 * bh + 1)) * int(rng.choice([1, 1, 500]))
    while ext[2] // bh + 1 > MAX_BINS:
        bh *= 7
    w, h = int(ext[0] // b + 2), int(ext[1] // b + 2)
    p = dict(bin=int(b), bin_height=bh, extent=[int(v) for v in ext])
    fp = _footprint_params(rng, w * h)
    if sparse:
        fp.update(threshold=int(rng.choice([0, 1, 10, 100])), kernel_size=int(rng.choice([1, 3])),
                  iterations=int(rng.choice([0, 0, 1])))
    p.update(fp)
    p["order"] = ("given", "random", "spatial", "pixel")[int(rng.integers(0, 4))]
    p["order_seed"] = int(rng.integers(0, 2**31))
    p["tail"] = int(rng.integers(1, 64)) if (n >= 128 and rng.random() < 0.5) else 0
    p["th2"] = ("negative", "zero", "fraction", "above_all")[int(rng.integers(0, 4))]
    p["th2_u"] = float(rng.random())
    p["vote_regime"] = ("lds", "dense", "sorted")[int(rng.integers(0, 3))]
    p["vote_u"] = float(rng.random())
    p["vote_seed"] = int(rng.integers(0, 2**31))
    return p


def ordered_cloud(case, p):
    """The cloud in the point order of its parameters.  tail = t: the cloud is cut to n % 64 == t and its last t points
    become copies of one point at other heights, so that the last, partial wave lies in one pixel."""
    xyz = case["xyz"]
    rng = np.random.default_rng(p["order_seed"])
    if p["order"] == "random":
        xyz = xyz[rng.permutation(len(xyz))]
    elif p["order"] == "spatial":  # coarse cells in raster order, the generated order inside a cell
        c = int(rng.choice([300, 2000]))
        xyz = xyz[np.lexsort((xyz[:, 0] // c, xyz[:, 1] // c))]
    elif p["order"] == "pixel":
        key = (xyz[:, 1] // p["bin"]).astype(np.int64) * (p["extent"][0] // p["bin"] + 2) + xyz[:, 0] // p["bin"]
        xyz = xyz[np.argsort(key, kind="stable")]
    xyz = np.array(xyz, dtype=np.int32, order="C")
    t = p["tail"]
    if t:
        n = (len(xyz) - t) // 64 * 64 + t
        top = xyz[:n - t, 2].argmax()  # a point of the highest structure
        xyz = xyz[:n].copy()
        xyz[n - t:] = xyz[top]
        xyz[n - t:, 2] = rng.integers(0, int(xyz[top, 2]) + 1, t)
    return xyz


def second_threshold(p, xyz):
    z = xyz[:, 2].astype(np.float64)
    u = p["th2_u"]
    return {"negative": -1.0 - 5000.0 * u, "zero": 0.0, "fraction": float(np.quantile(z, u)) + 0.5,
            "above_all": float(z.max()) + 1.0 + u}[p["th2"]]


def extreme_heights(p, n):
    """z at and next to the int32 limits, and a threshold between them (the figures only: the raster needs z >= 0)"""
    rng = np.random.default_rng([p["vote_seed"], 1])
    z = rng.choice(np.array([I32_MIN, I32_MIN + 1, I32_MAX, I32_MAX - 1, -1, 0, 1], np.int64), n).astype(np.int32)
    th = float(rng.choice([float(I32_MIN), float(I32_MIN) + 0.5, -0.5, 0.0, float(I32_MAX) - 0.5, float(I32_MAX)]))
    return z, th


def plane_labels(p, n, n_buildings):
    """(plane_idx int32 [n], n_planes): n_planes puts the vote table (n_planes * (n_buildings + 1) cells) into the
    drawn regime; the labels include 0, -1 and labels above n_planes."""
    cols = n_buildings + 1
    lo, hi = {"lds": (1, VOTE_LDS_CELLS), "dense": (VOTE_LDS_CELLS + 1, VOTE_DENSE_CELLS),
              "sorted": (VOTE_DENSE_CELLS + 1, MAX_VOTE_CELLS)}[p["vote_regime"]]
    cells = np.exp(np.log(lo) + p["vote_u"] * (np.log(hi) - np.log(lo)))
    n_planes = max(int(cells) // cols, 1)
    if p["vote_regime"] != "lds":
        while n_planes * cols < lo:
            n_planes += 1
    rng = np.random.default_rng([p["vote_seed"], 2])
    distinct = min(n_planes, max(int(n * rng.uniform(0.02, 0.6)), 1))  # few points per plane: ties are common
    plane = rng.integers(-1, distinct + 3, n)
    if distinct < n_planes:  # spread over the whole table
        plane = np.where(plane >= 1, (plane * (n_planes // distinct)).clip(max=n_planes + 2), plane)
    return np.ascontiguousarray(plane.astype(np.int32)), n_planes


def full_image(ch1):
    """[h][w][3] around channel 1; channels 0 and 2 hold values no stage may read"""
    img = np.empty(ch1.shape + (3,), np.float64)
    img[..., 0], img[..., 1], img[..., 2] = 7e300, ch1, np.nan
    return img


def _sub_seed(rng):
    return int(rng.integers(0, 2**63))


def build_case(sub):
    rng = np.random.default_rng(sub)
    case = make_case(rng)
    return case, draw_params(rng, case)


def replay_case(seed, index):
    """Case `index` of the sequence of `seed`, the way --only reaches it: (case dict, params dict)."""
    rng = np.random.default_rng(seed)
    for _ in range(index + 1):
        sub = _sub_seed(rng)
    return build_case(sub)


# ---- the reference chain and the regimes a case reaches (no device) ------------------------------------------------

def vote_counts(plane, bidx, n_planes, nb):
    sel = (plane >= 1) & (plane <= n_planes) & (bidx >= 0)
    c = np.bincount((plane[sel].astype(np.int64) - 1) * max(nb, 1) + bidx[sel], minlength=n_planes * max(nb, 1))
    return c.reshape(n_planes, max(nb, 1))


def regimes(case, p, O=None):
    """The set of regimes the case reaches, from the references alone (the chain the device is compared with)."""
    import building_ref as bref
    import ref
    out = {"kind:" + case["sub"].split("+")[0]}
    if case["kind"] == "cloud":
        if O is None:
            from oracle import oracle as O
        xyz = ordered_cloud(case, p)
        n = len(xyz)
        out |= {"order:" + p["order"], "second_threshold:" + p["th2"]}
        img, th = O.grid_picture(xyz, extent=p["extent"], bin=p["bin"], bin_height=p["bin_height"])
        if int(xyz[:, 2].max()) // p["bin_height"] + 1 > ZH_LDS:
            out.add("height_bins>4096")
        if th / p["bin_height"] >= ZH_LDS:
            out.add("ground_th_bin>=4096")
        if n < 64:
            out.add("n<64")
    else:
        img = full_image(case["ch1"])
        if not np.isfinite(case["ch1"]).all():
            out.add("non_finite_pixel")
    kw = dict(threshold=p["threshold"], kernel_size=p["kernel_size"], iterations=p["iterations"])
    q = quantised(img[..., 1])
    if not np.array_equal(q > p["threshold"], img[..., 1] != 0):
        out.add("mask!=nonzero")
    if (q == p["threshold"]).any() and (q == p["threshold"] + 1).any():
        out.add("q==thr_and_thr+1")
    out.add(f"padded_width%64=={(img.shape[1] + 2) % 64}")
    if img.shape[0] * img.shape[1] > LARGE_IMAGE:
        out.add("large_image")
    _, mask = ref.footprints(img, **kw)
    b = bref.building_map(mask)
    nb = b.n_buildings
    if nb > FIG_CAP:
        out.add("buildings>256")
    if nb == 0:
        out.add("buildings==0")
    if (b.pixels > b.fg_pixels).any():
        out.add("courtyard")
    if case["kind"] == "cloud":
        a = bref.assign(xyz, b.map, nb, p["bin"], th)
        t = n % 64
        if t and a.building_idx[-1] >= 0 and (a.building_idx[n - t:] == a.building_idx[-1]).all():
            out.add("tail_in_a_building")
        plane, n_planes = plane_labels(p, n, nb)
        cells = n_planes * (nb + 1)
        out.add("votes_lds" if cells <= VOTE_LDS_CELLS else "votes_dense" if cells <= VOTE_DENSE_CELLS else "votes_sorted")
        if nb:
            c = vote_counts(plane, a.building_idx, n_planes, nb)
            top = c.max(1)
            if ((c == top[:, None]).sum(1)[top > 0] > 1).any():
                out.add("vote_tie")
    return out


REGIMES = ("height_bins>4096", "ground_th_bin>=4096", "buildings>256", "buildings==0", "mask!=nonzero",
           "q==thr_and_thr+1", "non_finite_pixel", "courtyard", "vote_tie", "votes_lds", "votes_dense", "votes_sorted",
           "padded_width%64==0", "padded_width%64==1", "padded_width%64==63", "n<64", "tail_in_a_building", "large_image")
# reached at least once: every kind of cloud and image, every point order, every kind of second threshold
VARIANTS = tuple("kind:" + k for k in CLOUD_KINDS + IMAGE_KINDS) + \
    tuple("order:" + k for k in ("given", "random", "spatial", "pixel")) + \
    tuple("second_threshold:" + k for k in ("negative", "zero", "fraction", "above_all"))


def missing(hit):
    """what a run with these counts still lacks: every regime in three cases, every variant in one"""
    return [r for r in REGIMES if hit[r] < 3] + [v for v in VARIANTS if hit[v] < 1]


def coverage(seed, cases):
    """({regime: number of cases of the sequence that reach it}, the list of (case, params), the regimes of every
    case) -- CPU only"""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    hit = {r: 0 for r in REGIMES + VARIANTS}
    built, per_case = [], []
    for _ in range(cases):
        case, p = build_case(_sub_seed(rng))
        per_case.append(regimes(case, p, O) & set(hit))
        for r in per_case[-1]:
            hit[r] += 1
        built.append((case, p))
    return hit, built, per_case


# ---- device against reference ------------------------------------------------------------------------------------

class Check:
    def __init__(self):
        self.why = []

    def eq(self, stage, name, got, want):
        ok = (np.asarray(got).shape == np.asarray(want).shape and np.asarray(got).dtype == np.asarray(want).dtype
              and np.array_equal(got, want, equal_nan=True))
        if not ok:
            self.why.append(f"{stage}:{name}")
        return ok

    def true(self, stage, name, cond):
        if not cond:
            self.why.append(f"{stage}:{name}")


def same_footprints(ck, stage, fp, r):
    ck.true(stage, "n_contours", len(fp.contours) == len(r.contours))
    if len(fp.contours) == len(r.contours):
        ck.true(stage, "contours", all(np.array_equal(a, b) for a, b in zip(fp.contours, r.contours)))
        ck.eq(stage, "area", fp.area, r.area)
        ck.eq(stage, "perimeter", fp.perimeter, r.perimeter)


def check_footprints_and_map(ctx, ck, img, kw):
    """stages footprints and building map on one image; returns (bmap, Buildings, record of the device arrays)"""
    import building_ref as bref
    import ref
    fp, mask = ctx.footprints(img, return_mask=True, **kw)
    r, rmask = ref.footprints(img, **kw)
    ck.eq("footprints", "mask", mask, rmask * 255)
    same_footprints(ck, "footprints", fp, r)
    bmap, b = ctx.building_map(mask)
    rb = bref.building_map(mask)
    ck.true("map", "n_buildings", b.n_buildings == rb.n_buildings and (b.width, b.height) == (rb.width, rb.height))
    ck.eq("map", "map", bmap, rb.map)
    for k in bref.PIXEL_FIGURES:
        ck.eq("map", k, getattr(b, k), getattr(rb, k))
    ck.true("map", "contour_count", b.n_buildings == len(fp.contours))  # building c is contour c of the device's trace
    if b.n_buildings == len(fp.contours):
        ck.true("map", "contour_start", all(tuple(c[0]) == tuple(s) for c, s in zip(fp.contours, b.start_xy)))
        ck.true("map", "contour_on_building", all((bmap[c[:, 1], c[:, 0]] == i).all() for i, c in enumerate(fp.contours)))
    rec = [mask, bmap, fp.area, fp.perimeter] + list(fp.contours) + [getattr(b, k) for k in bref.PIXEL_FIGURES]
    return bmap, b, rec


def run_cloud(ctx, O, case, p, ck):
    import building_ref as bref
    xyz = ordered_cloud(case, p)
    n = len(xyz)
    rk = dict(extent=p["extent"], bin=p["bin"], bin_height=p["bin_height"])
    img, th = ctx.grid_picture(xyz, **rk)
    oimg, oth = O.grid_picture(xyz, **rk)
    ck.eq("raster", "image", img, oimg)
    ck.true("raster", f"ground_th={th}vs{oth}", th == oth)
    kw = dict(threshold=p["threshold"], kernel_size=p["kernel_size"], iterations=p["iterations"])
    bmap, b, rec = check_footprints_and_map(ctx, ck, img, kw)
    rec += [img, np.float64(th)]
    nb = b.n_buildings
    zx, thx = extreme_heights(p, n)
    pts_x = xyz.copy()
    pts_x[:, 2] = zx
    for name, pts, g in (("assign", xyz, th), ("assign_th2", xyz, second_threshold(p, xyz)), ("assign_int32", pts_x, thx)):
        bidx = ctx.assign_buildings(pts, bmap, b, bin=p["bin"], ground_th=g)
        a = bref.assign(pts, bmap, nb, p["bin"], g)
        ck.eq(name, "building_idx", bidx, a.building_idx)
        for k in bref.POINT_FIGURES:
            ck.eq(name, k, getattr(b, k), getattr(a, k))
        rec += [bidx] + [getattr(b, k).copy() for k in bref.POINT_FIGURES]
        if name == "assign":
            bidx0 = bidx
    plane, n_planes = plane_labels(p, n, nb)
    v = ctx.plane_buildings(plane, bidx0, n_planes, nb)
    want = bref.votes(plane, bidx0, n_planes, nb)
    got = (v.plane_building, v.votes_in, v.votes_total, v.votes_outside)
    for g_, w_, k in zip(got, want, ("plane_building", "votes_in", "votes_total", "votes_outside")):
        ck.eq("votes", k, g_, w_)
    rec += list(got)
    return rec, f"n={n} bin={p['bin']} bh={p['bin_height']} {img.shape[1]}x{img.shape[0]} th={th} nb={nb} planes={n_planes}"


def run_image(ctx, case, p, ck):
    img = full_image(case["ch1"])
    bmap, b, rec = check_footprints_and_map(ctx, ck, img, p)
    return rec, f"{img.shape[1]}x{img.shape[0]} nb={b.n_buildings}"


def same_records(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def tall_tile(rng):
    n = int(rng.integers(500, 5000))
    top = int(rng.uniform(2e6, 5e6))
    z = top - rng.integers(0, top, n) // 20
    pts = np.concatenate([rng.integers(0, 3000, (n, 2)), z[:, None]], 1)
    pts -= pts.min(0, keepdims=True)
    return np.ascontiguousarray(pts.astype(np.int32))


def run_batch(ctx, O, group, brng, ck, repeat=1):
    """The cases of `group` as tiles: the clouds through grid_picture_batch (a tall tile in the middle), their rasters
    and the images through footprints_batch (an empty tile in the middle).  One bin / bin_height / footprint
    parameter set per batch: the coarsest bin and the finest height bin of the group, the first case's footprint
    parameters bounded for the largest tile.  brng: the generator of this batch's extra tiles.  repeat: device runs
    of each batch call; every run must give identical arrays."""
    import ref
    clouds = [(ordered_cloud(c, p), p) for c, p in group if c["kind"] == "cloud"]
    images = [full_image(c["ch1"]) for c, p in group if c["kind"] == "image"]
    if clouds:
        bin_ = max(p["bin"] for _, p in clouds)
        bh = min(p["bin_height"] for _, p in clouds)
        tiles = [x for x, _ in clouds]
        exts = [np.maximum(np.asarray(p["extent"]), x.max(0)) for x, p in clouds]
        tall = tall_tile(brng)
        tiles.insert(len(tiles) // 2 + (len(tiles) == 1), tall)
        exts.insert(len(exts) // 2 + (len(exts) == 1), tall.max(0))
        while max(int(e[2]) // bh + 1 for e in exts) > MAX_BINS:
            bh *= 7
        exts = np.asarray(exts, dtype=np.int32)
        res = ctx.grid_picture_batch(tiles, extents=exts, bin=bin_, bin_height=bh)
        for _ in range(repeat - 1):
            again = ctx.grid_picture_batch(tiles, extents=exts, bin=bin_, bin_height=bh)
            ck.true("repeat", "raster_batch_runs_differ",
                    all(ta == tb and np.array_equal(ia, ib, equal_nan=True) for (ia, ta), (ib, tb) in zip(res, again)))
        for t, (img, th) in enumerate(res):
            oimg, oth = O.grid_picture(tiles[t], extent=exts[t], bin=bin_, bin_height=bh)
            simg, sth = ctx.grid_picture(tiles[t], extent=exts[t], bin=bin_, bin_height=bh)
            ck.eq(f"raster_batch[{t}]", "image_vs_oracle", img, oimg)
            ck.eq(f"raster_batch[{t}]", "image_vs_solo", img, simg)
            ck.true(f"raster_batch[{t}]", f"ground_th={th}vs{oth}vs{sth}", th == oth == sth)
            images.append(img)
    images.insert(len(images) // 2 + (len(images) == 1), np.zeros((int(brng.integers(1, 40)), int(brng.integers(1, 90)), 3)))
    kw = {k: group[0][1][k] for k in ("threshold", "kernel_size", "iterations")}
    kw["kernel_size"], kw["iterations"] = _bound_closing(max(i.shape[0] * i.shape[1] for i in images) * 1.5,
                                                         kw["kernel_size"], kw["iterations"])
    fps, masks = ctx.footprints_batch(images, return_mask=True, **kw)
    for _ in range(repeat - 1):
        fps2, masks2 = ctx.footprints_batch(images, return_mask=True, **kw)
        ck.true("repeat", "footprints_batch_masks_differ", all(np.array_equal(x, y) for x, y in zip(masks, masks2)))
        for t in range(len(images)):
            same_footprints(ck, f"repeat:footprints_batch[{t}]", fps2[t], fps[t])
    for t, img in enumerate(images):
        r, rmask = ref.footprints(img, **kw)
        sfp, smask = ctx.footprints(img, return_mask=True, **kw)
        ck.eq(f"footprints_batch[{t}]", "mask_vs_ref", masks[t], rmask * 255)
        ck.eq(f"footprints_batch[{t}]", "mask_vs_solo", masks[t], smask)
        same_footprints(ck, f"footprints_batch[{t}]_vs_ref", fps[t], r)
        same_footprints(ck, f"footprints_batch[{t}]_vs_solo", fps[t], sfp)
    return (f"raster_tiles={len(clouds) + bool(clouds)} footprint_tiles={len(images)} "
            + (f"bin={bin_} bh={bh} " if clouds else "") + " ".join(f"{k}={v}" for k, v in kw.items()))


def dump(args, case_no, case, p):
    arrs = {"xyz": case["xyz"]} if case["kind"] == "cloud" else {"ch1": case["ch1"]}
    np.savez_compressed(os.path.join(args.dump, f"fuzz_stages_fail_{args.seed}_{case_no}.npz"), params=json.dumps(p), **arrs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=GPU_TEST_CASES)
    ap.add_argument("--seed", type=int, default=GPU_TEST_SEED)
    ap.add_argument("--log", default="")
    ap.add_argument("--dump", default="", help="directory for the inputs of failing cases")
    ap.add_argument("--only", type=int, default=-1, help="run just this case of the sequence (the others are only drawn); with --batch: the batch that holds it")
    ap.add_argument("--repeat", type=int, default=1,
                    help="device runs per case (with --batch: per batch call): every run must give identical arrays")
    ap.add_argument("--batch", action="store_true",
                    help="runs of consecutive cases as the tiles of grid_picture_batch / footprints_batch")
    args = ap.parse_args()
    from buildingsegment_amd import api
    from oracle import oracle as O
    ctx = api.Context(0)
    rng = np.random.default_rng(args.seed)
    # --batch: the group sizes come from a stream of their own, drawn whether a batch runs or not (--only keeps the
    # batches where they are); the extra tiles of a batch come from a generator seeded with its first case
    brng = np.random.default_rng([args.seed, 0x626174])
    log = open(args.log, "a") if args.log else sys.stdout
    bad = 0
    t0 = time.time()
    group, left, first = [], 0, 0
    for case_no in range(args.cases):
        sub = _sub_seed(rng)
        if args.batch:
            if not group:
                left, first = int(brng.integers(2, 6)), case_no
            case, p = build_case(sub)
            group.append((case, p))
            pix = sum(c["ch1"].size if c["kind"] == "image" else 0 for c, _ in group)
            if len(group) < left and pix < 8_000_000 and case_no != args.cases - 1:
                continue
            ck = Check()
            if args.only < 0 or first <= args.only <= case_no:
                try:
                    desc = run_batch(ctx, O, group, np.random.default_rng([args.seed, first]), ck, args.repeat)
                except api.BsError as e:
                    desc = ""
                    ck.why.append(f"error:{e}")
                if ck.why and args.dump:
                    for k, (c, q) in enumerate(group):
                        dump(args, first + k, c, q)
                bad += bool(ck.why)
                print(f"cases {first}-{case_no} batch {desc} {'ok' if not ck.why else 'MISMATCH ' + ' '.join(ck.why)}",
                      file=log, flush=True)
            group = []
            continue
        if args.only >= 0 and case_no != args.only:  # the stream is already in step: one draw per case
            continue
        case, p = build_case(sub)
        ck = Check()
        desc = ""
        try:
            recs = []
            for _ in range(args.repeat):
                rec, desc = run_cloud(ctx, O, case, p, ck) if case["kind"] == "cloud" else run_image(ctx, case, p, ck)
                recs.append(rec)
            ck.true("repeat", "runs_differ", all(same_records(recs[0], r) for r in recs[1:]))
        except api.BsError as e:
            ck.why.append(f"error:{e}")
        if ck.why and args.dump:
            dump(args, case_no, case, p)
        bad += bool(ck.why)
        fk = {k: p[k] for k in ("threshold", "kernel_size", "iterations")}
        print(f"case {case_no} {case['kind']}/{case['sub']} {desc} thr={fk['threshold']} ks={fk['kernel_size']} "
              f"it={fk['iterations']} {'ok' if not ck.why else 'MISMATCH ' + ' '.join(sorted(set(ck.why)))}",
              file=log, flush=True)
    print(f"done: {args.cases} cases, {bad} mismatches, 0 skipped, {time.time() - t0:.1f} s", file=log, flush=True)
    ctx.close()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
