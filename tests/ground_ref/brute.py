"""The ground stage by its definition (include/bs_api.h, "ground"): Python integers, a loop over every window of every pixel
of every step.  Slow and plain on purpose; tests/ground_ref/ground_ref.py is checked against it."""
EMPTY = 2 ** 31 - 1
MAX_STEPS = 16
MAX_RADIUS = 255
COORD_LIMIT = 1 << 23
FIGURES = ("n_ground_pixels", "n_object_pixels", "n_empty_pixels", "n_filled_pixels", "n_ground_points", "n_low_points",
           "n_object_points", "dtm_min", "dtm_max", "hag_min", "hag_max", "sum_hag_ground")
PARAMS = ("cell", "radius", "s_num", "s_den", "dh0", "dh_max", "tol", "min_height")


class InvalidError(ValueError):
    """BS_ERR_INVALID of the definition"""


class RangeError(ValueError):
    """BS_ERR_RANGE of the definition"""


def grid_dims(extent, cell):
    return int(extent[0]) // cell + 2, int(extent[1]) // cell + 2


def thresholds(p):
    out, prev = [], 0
    for r in p["radius"]:
        out.append(min(p["dh_max"], p["dh0"] + (p["s_num"] * (r - prev) * p["cell"]) // p["s_den"]))
        prev = r
    return out


def check(xyz, extent, p):
    """the errors of the definition, in its order: (width, height)"""
    if xyz is None or extent is None or p is None:
        raise InvalidError("null")
    if len(xyz) < 1 or p["cell"] < 1:
        raise InvalidError("n < 1 or cell < 1")
    if int(extent[0]) < 0 or int(extent[1]) < 0:
        raise InvalidError("extent")
    rad = list(p["radius"])
    if not 1 <= len(rad) <= MAX_STEPS:
        raise InvalidError("n_steps")
    for k, r in enumerate(rad):
        if not 1 <= r <= MAX_RADIUS or (k and r <= rad[k - 1]):
            raise InvalidError("radius")
    if p["s_num"] < 0 or p["s_den"] < 1:
        raise InvalidError("slope")
    if min(p["dh0"], p["dh_max"], p["tol"], p["min_height"]) < 0:
        raise InvalidError("negative")
    if len(xyz) >= 1 << 29:
        raise RangeError("points")
    w, h = grid_dims(extent, p["cell"])
    if w * h >= 2 ** 31 - 1:
        raise RangeError("pixels")
    return w, h


def window(img, w, h, x, y, r, pick):
    """pick (min or max) over the square around (x, y) clipped to the image, ignoring EMPTY; EMPTY if all are"""
    vals = []
    for yy in range(max(0, y - r), min(h - 1, y + r) + 1):
        vals += [v for v in img[yy][max(0, x - r):min(w - 1, x + r) + 1] if v != EMPTY]
    return pick(vals) if vals else EMPTY


def ground(xyz, extent, p):
    """dict: width, height, threshold, step_pixels, low, dtm, step (lists of rows), hag, cls (lists) and FIGURES"""
    w, h = check(xyz, extent, p)
    cell = p["cell"]
    pts = [(int(a), int(b), int(c)) for a, b, c in xyz]
    for x, y, z in pts:
        if x < 0 or y < 0 or x // cell >= w or y // cell >= h:
            raise RangeError("xy")
    for x, y, z in pts:
        if max(abs(x), abs(y), abs(z)) >= COORD_LIMIT:
            raise RangeError("coordinate")
    low = [[EMPTY] * w for _ in range(h)]
    for x, y, z in pts:
        low[y // cell][x // cell] = min(low[y // cell][x // cell], z)
    S = [row[:] for row in low]
    step = [[255 if v == EMPTY else 0 for v in row] for row in low]
    th = thresholds(p)
    step_pixels = []
    for k, r in enumerate(p["radius"], 1):
        E = [[window(S, w, h, x, y, r, min) for x in range(w)] for y in range(h)]
        O = [[window(E, w, h, x, y, r, max) for x in range(w)] for y in range(h)]
        cnt = 0
        for y in range(h):
            for x in range(w):
                if step[y][x] == 0 and S[y][x] != EMPTY and S[y][x] - O[y][x] > th[k - 1]:
                    step[y][x] = k
                    cnt += 1
        step_pixels.append(cnt)
        S = O
    dtm = [[low[y][x] if step[y][x] == 0 else S[y][x] for x in range(w)] for y in range(h)]
    hag, cls = [], []
    for x, y, z in pts:
        g = z - dtm[y // cell][x // cell]
        hag.append(g)
        cls.append(0 if step[y // cell][x // cell] == 0 and g <= p["tol"] else (2 if g >= p["min_height"] else 1))
    flat = lambda img: [v for row in img for v in row]  # noqa: E731
    fl, fd, fs = flat(low), flat(dtm), flat(step)
    have = [v for v in fd if v != EMPTY]
    out = dict(width=w, height=h, threshold=th, step_pixels=step_pixels, low=low, dtm=dtm, step=step, hag=hag, cls=cls)
    out.update(n_ground_pixels=sum(s == 0 for s in fs), n_object_pixels=sum(0 < s < 255 for s in fs),
               n_empty_pixels=sum(v == EMPTY for v in fl),
               n_filled_pixels=sum(a == EMPTY and b != EMPTY for a, b in zip(fl, fd)),
               n_ground_points=cls.count(0), n_low_points=cls.count(1), n_object_points=cls.count(2),
               dtm_min=min(have) if have else EMPTY, dtm_max=max(have) if have else -2 ** 31,
               hag_min=min(hag), hag_max=max(hag), sum_hag_ground=sum(g for g, c in zip(hag, cls) if c == 0))
    return out
