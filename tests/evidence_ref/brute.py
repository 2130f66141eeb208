"""Roof evidence by its definition (include/bs_api.h, "roof evidence"): Python integers, one loop over the points, one loop
per pixel and window.  Slow and plain on purpose; tests/evidence_ref/evidence_ref.py is checked against it."""
EMPTY = 2 ** 31 - 1
RMAX = 15
FIGURES = ("n_counted", "n_planar", "n_pixels", "pixels_kept", "pixels_rejected", "pixels_thin", "max_window")
IMAGES = ("keep", "above", "planar", "win_above", "win_planar")


class InvalidError(ValueError):
    """BS_ERR_INVALID of the definition"""


class RangeError(ValueError):
    """BS_ERR_RANGE of the definition"""


def grid_dims(extent, bin):
    return int(extent[0]) // bin + 2, int(extent[1]) // bin + 2


def params(r=3, min_points=1, share=(1, 2)):
    return dict(r=int(r), min_points=int(min_points), num=int(share[0]), den=int(share[1]))


def check(xyz, plane_idx, n_planes, plane_ok, extent, bin, p):
    """the errors of the definition that need no look at a point, in its order: (width, height)"""
    if xyz is None or plane_idx is None or extent is None or p is None:
        raise InvalidError("null")
    if len(xyz) < 1 or len(plane_idx) != len(xyz) or bin < 1 or n_planes < 0:
        raise InvalidError("n < 1, bin < 1 or n_planes < 0")
    if plane_ok is not None and len(plane_ok) != n_planes:
        raise InvalidError("plane_ok")
    if int(extent[0]) < 0 or int(extent[1]) < 0:
        raise InvalidError("extent")
    if not 0 <= p["r"] <= RMAX or p["min_points"] < 1 or p["den"] < 1 or not 0 <= p["num"] <= p["den"]:
        raise InvalidError("parameters")
    if len(xyz) >= 1 << 29:
        raise RangeError("points")
    w, h = grid_dims(extent, bin)
    if w * h >= 2 ** 31 - 1:
        raise RangeError("pixels")
    return w, h


def below(x, y, z, ground_th, model):
    """the ground rule of a point: against the table where it holds a height for the point's model pixel, else z < ground_th"""
    if model is not None and x >= 0 and y >= 0:
        dtm, cell, min_height = model
        gx, gy = x // cell, y // cell
        if gy < len(dtm) and gx < len(dtm[0]):
            g = int(dtm[gy][gx])
            if g != EMPTY:
                return z < g + min_height
    return float(z) < ground_th


def evidence(xyz, plane_idx, n_planes, plane_ok, extent, bin, ground_th, p, model=None):
    """dict: width, height, the five images as lists of rows, and every name of FIGURES"""
    w, h = check(xyz, plane_idx, n_planes, plane_ok, extent, bin, p)
    above = [[0] * w for _ in range(h)]
    planar = [[0] * w for _ in range(h)]
    pts = [(int(a), int(b), int(c)) for a, b, c in xyz]
    for x, y, z in pts:
        if x < 0 or y < 0 or x // bin >= w or y // bin >= h:
            raise RangeError("xy")
    for (x, y, z), lab in zip(pts, plane_idx):
        if below(x, y, z, ground_th, model):
            continue
        lab = int(lab)
        above[y // bin][x // bin] += 1
        if 1 <= lab <= n_planes and (plane_ok is None or int(plane_ok[lab - 1]) != 0):
            planar[y // bin][x // bin] += 1
    r = p["r"]
    out = dict(width=w, height=h, above=above, planar=planar, keep=[[0] * w for _ in range(h)],
               win_above=[[0] * w for _ in range(h)], win_planar=[[0] * w for _ in range(h)])
    fig = dict.fromkeys(FIGURES, 0)
    for y in range(h):
        for x in range(w):
            A = P = 0
            for yy in range(max(0, y - r), min(h, y + r + 1)):
                for xx in range(max(0, x - r), min(w, x + r + 1)):
                    A += above[yy][xx]
                    P += planar[yy][xx]
            out["win_above"][y][x], out["win_planar"][y][x] = A, P
            enough, share = A >= p["min_points"], P * p["den"] >= p["num"] * A
            out["keep"][y][x] = int(enough and share)
            fig["n_counted"] += above[y][x]
            fig["n_planar"] += planar[y][x]
            fig["n_pixels"] += above[y][x] > 0
            fig["pixels_kept"] += enough and share
            fig["pixels_rejected"] += enough and not share
            fig["pixels_thin"] += 0 < A < p["min_points"]
            fig["max_window"] = max(fig["max_window"], A)
    out.update(fig)
    return out


def plane_quality(status, n_points, r_sq_sum, min_points=0, max_rms=100):
    """ok [n_planes] of bs_plane_quality"""
    if min_points < 0 or not 0 <= max_rms <= 32767:
        raise InvalidError("plane quality")
    return [int(int(s) == 0 and int(n) >= min_points and int(q) <= max_rms * max_rms * int(n))
            for s, n, q in zip(status, n_points, r_sq_sum)]
