"""Restatement of the plane fit (include/bs_api.h, "plane fit") in numpy and Python integers: what the device must
return, array for array, with ==.  Sums are numpy int64 (every one fits by the definition's own verdict), the verdict
is Python integer arithmetic, the covariance np.float64 (arrays in plane_fit, scalars in brute), the solve oracle.fast_eigen3x3 (the independent C
restatement of the solver the stage-2 normals are checked against) and the residuals numpy."""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ARRAYS = ("status", "n_points", "center", "normal", "bbox", "dev_sum", "moment", "r_abs_max", "r_abs_sum", "r_sq_sum")
DTYPES = dict(status=np.int32, n_points=np.int64, center=np.int32, normal=np.float64, bbox=np.int32, dev_sum=np.int64,
              moment=np.int64, r_abs_max=np.int32, r_abs_sum=np.int64, r_sq_sum=np.int64)


def tdiv(a, b):
    """C division of Python integers: truncated towards zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def verdict(n, center, lo, hi):
    """status of a plane with n > 0 points (Python integers throughout)"""
    if n < 3:
        return 1
    D = max(max(int(hi[a]) - center[a], center[a] - int(lo[a])) for a in range(3))
    return 2 if 3 * n * D * D >= 2 ** 63 else 0


def normal_of(n, dev_sum, moment, eigen=None):
    """step 5 for one fitted plane: np.float64 scalars, no contraction"""
    if eigen is None:
        from oracle import oracle as O
        eigen = O.fast_eigen3x3
    dn = np.float64(n)
    e = [np.float64(int(v)) / dn for v in dev_sum]
    m = [np.float64(int(v)) / dn for v in moment]
    c6 = [m[0] - e[0] * e[0], m[1] - e[0] * e[1], m[2] - e[0] * e[2], m[3] - e[1] * e[1], m[4] - e[1] * e[2],
          m[5] - e[2] * e[2]]
    v = [np.float64(t) for t in eigen(np.array(c6, np.float64))]
    if np.sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])) == 0.0:
        v = [np.float64(0), np.float64(0), np.float64(1)]
    if v[0] * 0.0 + (v[1] * 0.0 + v[2] * 1.0) < 0.0:
        v = [t * -1.0 for t in v]
    return v


def _by_plane(lab, n_planes):
    """stable order of the labelled points by plane, the planes present and where each one's run starts"""
    order = np.argsort(lab, kind="stable")
    slab = lab[order]
    present = np.unique(slab)
    return order, slab, present, np.searchsorted(slab, present)


def plane_fit(xyz, plane_idx, n_planes, eigen=None):
    xyz = np.asarray(xyz, np.int32).reshape(-1, 3)
    pi = np.asarray(plane_idx, np.int32)
    n, m = len(xyz), int(n_planes)
    assert pi.shape == (n,) and m >= 0 and 1 <= n < 2 ** 29 and np.abs(xyz.astype(np.int64)).max() < 2 ** 23
    f = SimpleNamespace(n_planes=m, **{k: np.zeros((m, {"center": 3, "normal": 3, "bbox": 6, "dev_sum": 3, "moment": 6}[k])
                                                  if k in ("center", "normal", "bbox", "dev_sum", "moment") else m, DTYPES[k])
                                       for k in ARRAYS})
    f.normal[:, 2] = 1.0
    f.bbox[:, :3], f.bbox[:, 3:] = I32_MAX, I32_MIN
    f.status[:] = 1
    f.residual = np.full(n, I32_MIN, np.int32)
    idx = np.nonzero((pi >= 1) & (pi <= m))[0]
    if m == 0 or len(idx) == 0:
        return f
    # 1. sums
    order, slab, present, starts = _by_plane(pi[idx] - 1, m)
    idx = idx[order]
    P = xyz[idx].astype(np.int64)
    f.n_points[:] = np.bincount(slab, minlength=m)
    S = np.zeros((m, 3), np.int64)
    S[present] = np.add.reduceat(P, starts, axis=0)
    f.bbox[present, :3] = np.minimum.reduceat(P, starts, axis=0)
    f.bbox[present, 3:] = np.maximum.reduceat(P, starts, axis=0)
    # 2. centroid and 3. verdict: Python integers
    Sl, nl, bl = S.tolist(), f.n_points.tolist(), f.bbox.tolist()
    for p in present.tolist():
        c = [tdiv(Sl[p][a], nl[p]) for a in range(3)]
        f.center[p] = c
        f.status[p] = verdict(nl[p], c, bl[p][:3], bl[p][3:])
    # 4. moments of the fitted planes (every sum fits int64 there, by the verdict)
    fitted = f.status[slab] == 0
    if not fitted.any():
        return f
    idx, slab, P = idx[fitted], slab[fitted], P[fitted]
    present = np.unique(slab)
    starts = np.searchsorted(slab, present)
    d = P - f.center[slab].astype(np.int64)
    f.dev_sum[present] = np.add.reduceat(d, starts, axis=0)
    prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                     d[:, 2] * d[:, 2]], 1)
    f.moment[present] = np.add.reduceat(prod, starts, axis=0)
    assert np.array_equal(f.dev_sum[present], S[present] - f.n_points[present, None] * f.center[present].astype(np.int64))
    # 5. normal: the covariance in np.float64 (elementwise: the scalar operations of normal_of, plane by plane)
    dn = f.n_points[present].astype(np.float64)
    e, mm = f.dev_sum[present].astype(np.float64) / dn[:, None], f.moment[present].astype(np.float64) / dn[:, None]
    c6 = np.stack([mm[:, 0] - e[:, 0] * e[:, 0], mm[:, 1] - e[:, 0] * e[:, 1], mm[:, 2] - e[:, 0] * e[:, 2],
                   mm[:, 3] - e[:, 1] * e[:, 1], mm[:, 4] - e[:, 1] * e[:, 2], mm[:, 5] - e[:, 2] * e[:, 2]], 1)
    if eigen is None:
        from oracle import oracle as O
        eigen = O.fast_eigen3x3
    v = np.array([eigen(c) for c in c6], np.float64).reshape(-1, 3)
    zero = np.sqrt(v[:, 0] * v[:, 0] + (v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])) == 0.0
    v[zero] = [0.0, 0.0, 1.0]
    flip = v[:, 0] * 0.0 + (v[:, 1] * 0.0 + v[:, 2] * 1.0) < 0.0
    v[flip] *= -1.0
    f.normal[present] = v
    # 6. residuals: nx * dx + (ny * dy + nz * dz) in f64, truncated
    nv, dd = f.normal[slab], d.astype(np.float64)
    r = np.trunc(nv[:, 0] * dd[:, 0] + (nv[:, 1] * dd[:, 1] + nv[:, 2] * dd[:, 2])).astype(np.int64)
    f.residual[idx] = r.astype(np.int32)
    a = np.abs(r)
    f.r_abs_max[present] = np.maximum.reduceat(a, starts)
    f.r_abs_sum[present] = np.add.reduceat(a, starts)
    f.r_sq_sum[present] = np.add.reduceat(a * a, starts)
    return f


def apply(f, normal, center):
    """bs_plane_fit_apply: new tables with the rows of the fitted planes replaced"""
    ok = f.status == 0
    return (np.where(ok[:, None], f.normal, np.asarray(normal, np.float64).reshape(-1, 3)),
            np.where(ok[:, None], f.center, np.asarray(center, np.int32).reshape(-1, 3)).astype(np.int32))


def height_of(normal, center, X, Y):
    """H(p, X, Y) of the roof stage without its clamps (include/bs_api.h, roofs, step 5) for one plane, f64"""
    t = normal[0] * (np.asarray(X, np.float64) - np.float64(center[0])) + normal[1] * (np.asarray(Y, np.float64) - np.float64(center[1]))
    return np.float64(center[2]) - t / normal[2]


def brute(xyz, plane_idx, n_planes, eigen=None):
    """The same definition with per-plane lists and loops over Python integers; returns a dict of lists."""
    m = int(n_planes)
    pts = [[] for _ in range(m)]
    for i, l in enumerate(plane_idx):
        if 1 <= int(l) <= m:
            pts[int(l) - 1].append((i, tuple(int(v) for v in xyz[i])))
    out = {k: [] for k in ARRAYS}
    residual = [I32_MIN] * len(xyz)
    for p in range(m):
        cnt = len(pts[p])
        S = [sum(q[a] for _, q in pts[p]) for a in range(3)]
        lo = [min((q[a] for _, q in pts[p]), default=I32_MAX) for a in range(3)]
        hi = [max((q[a] for _, q in pts[p]), default=I32_MIN) for a in range(3)]
        c = [tdiv(S[a], cnt) if cnt else 0 for a in range(3)]
        st = verdict(cnt, c, lo, hi) if cnt else 1
        dev, mom, nv, rmax, rsum, rsq = [0] * 3, [0] * 6, [0.0, 0.0, 1.0], 0, 0, 0
        if st == 0:
            ds = [tuple(q[a] - c[a] for a in range(3)) for _, q in pts[p]]
            dev = [sum(d[a] for d in ds) for a in range(3)]
            mom = [sum(d[a] * d[b] for d in ds) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
            nv = normal_of(cnt, dev, mom, eigen)
            for (i, _), d in zip(pts[p], ds):
                r = int(nv[0] * np.float64(d[0]) + (nv[1] * np.float64(d[1]) + nv[2] * np.float64(d[2])))
                residual[i] = r
                rmax, rsum, rsq = max(rmax, abs(r)), rsum + abs(r), rsq + r * r
        for k, v in zip(ARRAYS, (st, cnt, c, [float(t) for t in nv], lo + hi, dev, mom, rmax, rsum, rsq)):
            out[k].append(v)
    out["residual"] = residual
    return out
