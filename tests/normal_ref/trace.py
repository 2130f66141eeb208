"""A third transcription of the normal's floating-point tail, in plain Python floats, that records the leaves it takes.

Written from SURVEY.md Appendix A.2 / A.3 (as oracle/bs_oracle.c and csrc/bs_normal.h were): every line below is one
IEEE double operation in the order given there, Python's float IS the IEEE double and never contracts a*b+c.  The
square roots are math.sqrt (correctly rounded, as the oracle's libm sqrt and the device's bs_det_sqrt are), the two
transcendental calls are the shared bs_detmath.h through the oracle.  Divisions go through _div, because Python raises
where IEEE returns an infinity or a NaN.

fast_eigen3x3(c6) -> (vector, leaves): the solver alone.  normal_of_cov / normal_of_points add the tail (zero-norm
fallback, orientation to +z).  cov_of is the cumulant covariance of A.2 in list order.

Leaves (see LEAVES): where the solver branches.  'clamp-' / 'clamp+' mean det / 2 <= -1 / >= 1.  Three leaves mark
comparisons that meet an equality, where "the first wins" is part of the specification: 'e0.tie' (the largest cross
product is not the only one of its length), 'e1.tie' (|m00| == |m11|), 'e1.tie01' (the larger of them == |m01|).
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEAVES = ("zero", "negmax", "diag.x", "diag.y", "diag.z", "clamp-", "clamp+", "h+", "h-", "e0.0", "e0.1", "e0.2", "e0.zero",
          "e0.tie", "e1.Ux", "e1.Uy", "e1.tie", "e1.tie01", "e1.a", "e1.b", "e1.c", "e1.d", "e1.U0", "e1.U1", "h+.v2", "h+.v1",
          "h+.x", "h-.v0", "h-.v1", "h-.x")

TWO_THIRDS_PI = 2.09439510239319549


def _detmath():
    from oracle import oracle as O
    O.lib()
    return O.det_acos, O.det_cos


def _div(a, b):
    """a / b as the hardware does it (x86 here: 0/0 is the NaN with the sign bit set, as in the C oracle)"""
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def _dot(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _eigvec0(A, l, leaves):
    r0 = [A[0] - l, A[1], A[2]]
    r1 = [A[1], A[3] - l, A[4]]
    r2 = [A[2], A[4], A[5] - l]
    x = [_cross(r0, r1), _cross(r0, r2), _cross(r1, r2)]
    d = [_dot(v, v) for v in x]
    dmax, imax = d[0], 0
    if d[1] > dmax:
        dmax, imax = d[1], 1
    if d[2] > dmax:
        imax = 2
    leaves.append("e0.zero" if d[imax] == 0 else "e0.%d" % imax)
    if d[imax] > 0 and any(d[j] == d[imax] for j in range(3) if j != imax):
        leaves.append("e0.tie")
    s = math.sqrt(d[imax])
    return [_div(x[imax][0], s), _div(x[imax][1], s), _div(x[imax][2], s)]


def _eigvec1(A, e, l, leaves):
    if abs(e[0]) > abs(e[1]):
        leaves.append("e1.Ux")
        s = _div(1.0, math.sqrt(e[0] * e[0] + e[2] * e[2]))
        U = [-e[2] * s, 0.0, e[0] * s]
    else:
        leaves.append("e1.Uy")
        s = _div(1.0, math.sqrt(e[1] * e[1] + e[2] * e[2]))
        U = [0.0, e[2] * s, -e[1] * s]
    V = _cross(e, U)
    AU = [A[0] * U[0] + A[1] * U[1] + A[2] * U[2], A[1] * U[0] + A[3] * U[1] + A[4] * U[2],
          A[2] * U[0] + A[4] * U[1] + A[5] * U[2]]
    AV = [A[0] * V[0] + A[1] * V[1] + A[2] * V[2], A[1] * V[0] + A[3] * V[1] + A[4] * V[2],
          A[2] * V[0] + A[4] * V[1] + A[5] * V[2]]
    m00 = U[0] * AU[0] + U[1] * AU[1] + U[2] * AU[2] - l
    m01 = U[0] * AV[0] + U[1] * AV[1] + U[2] * AV[2]
    m11 = V[0] * AV[0] + V[1] * AV[1] + V[2] * AV[2] - l
    a00, a01, a11 = abs(m00), abs(m01), abs(m11)
    if a00 == a11:
        leaves.append("e1.tie")
    if (a00 if a00 >= a11 else a11) == a01 and a01 > 0:
        leaves.append("e1.tie01")
    if a00 >= a11:
        mx = a00 if a00 > a01 else a01
        if mx > 0:
            if a00 >= a01:
                leaves.append("e1.a")
                m01 = _div(m01, m00)
                m00 = _div(1.0, math.sqrt(1 + m01 * m01))
                m01 = m01 * m00
            else:
                leaves.append("e1.b")
                m00 = _div(m00, m01)
                m01 = _div(1.0, math.sqrt(1 + m00 * m00))
                m00 = m00 * m01
            return [m01 * U[i] - m00 * V[i] for i in range(3)]
        leaves.append("e1.U0")
        return U
    mx = a11 if a11 > a01 else a01
    if mx > 0:
        if a11 >= a01:
            leaves.append("e1.c")
            m01 = _div(m01, m11)
            m11 = _div(1.0, math.sqrt(1 + m01 * m01))
            m01 = m01 * m11
        else:
            leaves.append("e1.d")
            m11 = _div(m11, m01)
            m01 = _div(1.0, math.sqrt(1 + m11 * m11))
            m11 = m11 * m01
        return [m11 * U[i] - m01 * V[i] for i in range(3)]
    leaves.append("e1.U1")
    return U


def fast_eigen3x3(c6):
    """c6 = (c00, c01, c02, c11, c12, c22) -> ([x, y, z], tuple of leaves)"""
    acos, cos = _detmath()
    c = [float(v) for v in c6]
    leaves = []
    m = c[0]
    for i in range(1, 6):
        if c[i] > m:
            m = c[i]
    if m == 0:
        return [0.0, 0.0, 0.0], ("zero",)
    if m < 0:
        leaves.append("negmax")
    A = [_div(v, m) for v in c]
    norm = A[1] * A[1] + A[2] * A[2] + A[4] * A[4]
    if norm > 0:
        q = (A[0] + A[3] + A[5]) / 3
        b00, b11, b22 = A[0] - q, A[3] - q, A[5] - q
        p = math.sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * 2) / 6)
        c00 = b11 * b22 - A[4] * A[4]
        c01 = A[1] * b22 - A[4] * A[2]
        c02 = A[1] * A[4] - b11 * A[2]
        det = _div(b00 * c00 - A[1] * c01 + A[2] * c02, p * p * p)
        h = det * 0.5
        if h <= -1.0:
            leaves.append("clamp-")
        if h >= 1.0:
            leaves.append("clamp+")
        h = h if h > -1.0 else -1.0
        h = h if h < 1.0 else 1.0
        angle = acos(h) / 3.0
        beta2 = cos(angle) * 2
        beta0 = cos(angle + TWO_THIRDS_PI) * 2
        beta1 = -(beta0 + beta2)
        e0, e1, e2 = q + p * beta0, q + p * beta1, q + p * beta2
        if h >= 0:
            leaves.append("h+")
            v2 = _eigvec0(A, e2, leaves)
            if e2 < e0 and e2 < e1:
                leaves.append("h+.v2")
                return v2, tuple(leaves)
            v1 = _eigvec1(A, v2, e1, leaves)
            if e1 < e0 and e1 < e2:
                leaves.append("h+.v1")
                return v1, tuple(leaves)
            leaves.append("h+.x")
            return _cross(v1, v2), tuple(leaves)
        leaves.append("h-")
        v0 = _eigvec0(A, e0, leaves)
        if e0 < e1 and e0 < e2:
            leaves.append("h-.v0")
            return v0, tuple(leaves)
        v1 = _eigvec1(A, v0, e1, leaves)
        if e1 < e0 and e1 < e2:
            leaves.append("h-.v1")
            return v1, tuple(leaves)
        leaves.append("h-.x")
        return _cross(v0, v1), tuple(leaves)
    d0, d1, d2 = A[0] * m, A[3] * m, A[5] * m
    if d0 < d1 and d0 < d2:
        return [1.0, 0.0, 0.0], tuple(leaves + ["diag.x"])
    if d1 < d0 and d1 < d2:
        return [0.0, 1.0, 0.0], tuple(leaves + ["diag.y"])
    return [0.0, 0.0, 1.0], tuple(leaves + ["diag.z"])


def cov_of(points):
    """A.2: the nine cumulants in f64, list order; fewer than 3 points -> the identity"""
    pts = [(float(int(p[0])), float(int(p[1])), float(int(p[2]))) for p in points]
    if len(pts) < 3:
        return [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    cu = [0.0] * 9
    for x, y, z in pts:
        cu[0] += x
        cu[1] += y
        cu[2] += z
        cu[3] += x * x
        cu[4] += x * y
        cu[5] += x * z
        cu[6] += y * y
        cu[7] += y * z
        cu[8] += z * z
    dn = float(len(pts))
    cu = [v / dn for v in cu]
    return [cu[3] - cu[0] * cu[0], cu[4] - cu[0] * cu[1], cu[5] - cu[0] * cu[2], cu[6] - cu[1] * cu[1],
            cu[7] - cu[1] * cu[2], cu[8] - cu[2] * cu[2]]


def normal_of_cov(c6):
    """the tail every normal goes through: solver, zero-norm fallback (0, 0, 1), orientation to +z"""
    v, leaves = fast_eigen3x3(c6)
    if math.sqrt(_dot(v, v)) == 0.0:
        v = [0.0, 0.0, 1.0]
    if v[0] * 0.0 + (v[1] * 0.0 + v[2] * 1.0) < 0.0:
        v = [t * -1.0 for t in v]
    return v, leaves


def normal_of_points(points):
    return normal_of_cov(cov_of(points))


def bits(v):
    """the 64-bit patterns of a vector (NaN sign and payload included)"""
    return np.asarray(v, np.float64).view(np.int64)
