"""The solids of include/bs_api.h ("solids") pixel by pixel in plain Python: dictionaries and lists, nothing vectorised.
Slow on purpose: this is the form that is read against the definition; tests/solid_ref/solid_ref.py is the fast one and
must equal it."""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "roof_ref"))
import roof_ref as rr  # noqa: E402

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
# wall d of a pixel: (s, e) as corners (i, j) of the pixel, the neighbour's offset, and which corners (i, j) of the
# neighbour the lattice points s and e are
WALLS = (((0, 0), (1, 0), (0, -1), (0, 1), (1, 1)),
         ((1, 0), (1, 1), (1, 0), (0, 0), (0, 1)),
         ((1, 1), (0, 1), (0, 1), (1, 0), (0, 0)),
         ((0, 1), (0, 0), (-1, 0), (1, 1), (1, 0)))


def solids(bmap, roof, n_buildings, normal, center, z_min, z_max, bin, base_z, flat):
    bmap, roof = np.asarray(bmap), np.asarray(roof)
    h, w = bmap.shape
    base_z = int(base_z)
    top = {}  # (x, y) -> {(i, j): height}
    for y in range(h):
        for x in range(w):
            c = int(bmap[y, x])
            if c < 0:
                continue
            t = {}
            for j in (0, 1):
                for i in (0, 1):
                    if roof[y, x] > 0:
                        z = int(rr.height_of(int(roof[y, x]), (x + i) * bin, (y + j) * bin, normal, center, z_min, z_max))
                    else:
                        z = int(flat[c])
                    t[i, j] = max(base_z, z)
            top[x, y] = t
    # vertices: per lattice corner and building, the distinct heights
    heights = {}  # (Y, X, c) -> set of heights
    for (x, y), t in top.items():
        c = int(bmap[y, x])
        for (i, j), z in t.items():
            heights.setdefault((y + j, x + i, c), {base_z}).add(z)
    vertex, number = [], {}
    for (Y, X, c) in sorted(heights):
        for z in sorted(heights[Y, X, c]):
            number[Y, X, c, z] = len(vertex)
            vertex.append((X * bin, Y * bin, z, c))

    def between(Y, X, c, z_from, z_to):
        lo, hi = min(z_from, z_to), max(z_from, z_to)
        mid = [z for z in sorted(heights[Y, X, c]) if lo < z < hi]
        return mid if z_from < z_to else mid[::-1]

    nb = n_buildings
    fig = SimpleNamespace(pixels=np.zeros(nb, np.int64), vertices=np.zeros(nb, np.int64), faces=np.zeros(nb, np.int64),
                          wall_faces=np.zeros(nb, np.int64), crossing_walls=np.zeros(nb, np.int64),
                          top_min=np.full(nb, I32_MAX, np.int32), top_max=np.full(nb, I32_MIN, np.int32),
                          volume6=np.zeros(nb, np.int64))
    for (Y, X, c), zs in heights.items():
        fig.vertices[c] += len(zs)
    faces, kinds, owners = [], [], []
    for y in range(h):
        for x in range(w):
            if (x, y) not in top:
                continue
            c, t = int(bmap[y, x]), top[x, y]

            def v(i, j, z):
                return number[y + j, x + i, c, z]

            mine = [([v(0, 0, t[0, 0]), v(1, 0, t[1, 0]), v(1, 1, t[1, 1])], 0),
                    ([v(0, 0, t[0, 0]), v(1, 1, t[1, 1]), v(0, 1, t[0, 1])], 0),
                    ([v(0, 0, base_z), v(0, 1, base_z), v(1, 1, base_z), v(1, 0, base_z)], 1)]
            for d, (s, e, (dx, dy), ns, ne) in enumerate(WALLS):
                a_s, a_e = t[s], t[e]
                nx, ny = x + dx, y + dy
                same = 0 <= nx < w and 0 <= ny < h and int(bmap[ny, nx]) == c
                if same and d in (0, 3):
                    continue  # the neighbour has the smaller index: the wall is its
                b_s, b_e = (top[nx, ny][ns], top[nx, ny][ne]) if same else (base_z, base_z)
                if (a_s, a_e) == (b_s, b_e):
                    continue
                poly = [(e, a_e), (s, a_s)] + [(s, z) for z in between(y + s[1], x + s[0], c, a_s, b_s)] + [(s, b_s), (e, b_e)]
                poly += [(e, z) for z in between(y + e[1], x + e[0], c, b_e, a_e)]
                kept = [p for k, p in enumerate(poly) if k == 0 or p != poly[k - 1]]  # (s, b_s) == (s, a_s) goes
                if kept[-1] == kept[0]:
                    kept.pop()  # (e, b_e) == (e, a_e) goes: the polygon starts at (e, a_e)
                assert 3 <= len(kept) <= 8
                mine.append(([v(i, j, z) for (i, j), z in kept], 2))
                fig.wall_faces[c] += 1
                fig.crossing_walls[c] += (a_s - b_s) * (a_e - b_e) < 0
            for idx, kind in mine:
                faces.append(idx)
                kinds.append(kind)
                owners.append(c)
            fig.pixels[c] += 1
            fig.faces[c] += len(mine)
            fig.top_min[c] = min(int(fig.top_min[c]), min(t.values()))
            fig.top_max[c] = max(int(fig.top_max[c]), max(t.values()))
            fig.volume6[c] += 2 * t[0, 0] + 2 * t[1, 1] + t[1, 0] + t[0, 1] - 6 * base_z
    img = np.full((h, w, 4), I32_MIN, np.int32)
    for (x, y), t in top.items():
        img[y, x] = [t[0, 0], t[1, 0], t[0, 1], t[1, 1]]
    off = np.zeros(len(faces) + 1, np.int32)
    off[1:] = np.cumsum([len(f) for f in faces]) if faces else []
    return SimpleNamespace(
        top=img, vertex=np.array(vertex, np.int32).reshape(-1, 4), face_offset=off,
        face_index=np.array([k for f in faces for k in f], np.int32), face_building=np.array(owners, np.int32),
        face_kind=np.array(kinds, np.uint8), n_buildings=nb, n_pixels=int(fig.pixels.sum()), n_vertices=len(vertex),
        n_faces=len(faces), n_indices=int(off[-1]), n_wall_faces=int(fig.wall_faces.sum()),
        n_crossing_walls=int(fig.crossing_walls.sum()), total_volume6=int(fig.volume6.sum()), **vars(fig))
