"""The smallest eigenvector at 60 digits (mpmath), two ways:

of_matrix(c6)   of the f64 covariance matrix the solver is handed: what the solver alone loses;
of_points(pts)  of the exact rational covariance of integer points (fractions): adds what the cumulants' cancellation
                c3 - c0 * c0 loses far from the origin.

Both return (eigenvector of the smallest eigenvalue, the three eigenvalues ascending) as mpmath numbers.
sin_angle(n, v) is |n x v| / (|n| |v|) at the same precision; gap_ok says whether the smallest eigenvalue is separated
from the next one well enough for the eigenvector to be a property of the matrix at all."""
from fractions import Fraction

from mpmath import mp, mpf

DPS = 60
GAP = mpf(10) ** -6      # lambda_1 - lambda_0 > GAP * lambda_2
EPS = mpf(2) ** -52


def _solve(rows):
    with mp.workdps(DPS):
        E, Q = mp.eigsy(mp.matrix(rows))
        order = sorted(range(3), key=lambda i: E[i])
        lam = [E[i] for i in order]
        v = [Q[r, order[0]] for r in range(3)]
        return v, lam


def of_matrix(c6):
    with mp.workdps(DPS):
        a = [mpf(float(t)) for t in c6]
        return _solve([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])


def exact_cov(points):
    """E[ab] - E[a] E[b] of integer points as six Fractions (c00, c01, c02, c11, c12, c22)"""
    pts = [tuple(int(t) for t in p) for p in points]
    n = len(pts)
    s = [sum(p[a] for p in pts) for a in range(3)]
    out = []
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        sab = sum(p[a] * p[b] for p in pts)
        out.append(Fraction(sab, n) - Fraction(s[a], n) * Fraction(s[b], n))
    return out


def of_points(points):
    with mp.workdps(DPS):
        a = [mpf(f.numerator) / mpf(f.denominator) for f in exact_cov(points)]
        return _solve([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])


def gap_ok(lam):
    with mp.workdps(DPS):
        return lam[1] - lam[0] > GAP * abs(lam[2])


def sin_angle(n, v):
    with mp.workdps(DPS):
        a = [mpf(float(t)) for t in n]
        c = [a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0]]
        num = mp.sqrt(c[0] ** 2 + c[1] ** 2 + c[2] ** 2)
        return num / (mp.sqrt(a[0] ** 2 + a[1] ** 2 + a[2] ** 2) * mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2))


def factor(n, v, lam):
    """sin(angle) in units of the eigenvector's condition: sin * (lambda_1 - lambda_0) / (lambda_2 * 2^-52)"""
    with mp.workdps(DPS):
        return sin_angle(n, v) * (lam[1] - lam[0]) / (abs(lam[2]) * EPS)
