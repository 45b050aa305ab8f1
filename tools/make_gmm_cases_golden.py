"""Writes tests/golden/gmm_cases_exact.npz: the 60-digit reference values of tests/gmm_cases.py.

Everything is computed with mpmath at 60 digits on the exact binary values of each case's inputs and rounded to double
at the end, so no value shares a rounding with the code under test (the CPU oracle runs the same Jacobi, cofactor inverse
and Cholesky as the kernels).  Per BUILD case (rows in the order of gmm_cases.BUILD; NaN where the input is not finite):
  build_w      eigenvalues of the LOWER triangle, ascending      build_wu   the same for the UPPER triangle
  build_inv    inverse of the full matrix                         build_det  its determinant
  build_chol   lower Cholesky factor of the inverse's lower triangle (NaN where it is not positive definite)
  build_plane  unit eigenvector of the smallest lower-triangle eigenvalue (largest component positive) and n . mean
Per GRAPH case: graph_<name>, the K x K Bhattacharyya distances (NaN on the diagonal and where the formula has no value).
The archive is written with fixed timestamps and no compression: the same inputs give the same bytes
(tests/test_gmm_cases.py::test_golden_regenerates_byte_identically).

Usage: python tools/make_gmm_cases_golden.py [output path]
"""
import io
import os
import sys
import zipfile
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEFAULT = os.path.join(ROOT, "tests", "golden", "gmm_cases_exact.npz")


def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath


def _mat(mp, a):
    return mp.matrix([[mp.mpf(float(a[i, j])) for j in range(3)] for i in range(3)])


def _sym(mp, A, lower):
    S = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            S[i, j] = A[max(i, j), min(i, j)] if lower else A[min(i, j), max(i, j)]
    return S


def _det(A):
    return (A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) - A[0, 1] * (A[1, 0] * A[2, 2] - A[1, 2] * A[2, 0])
            + A[0, 2] * (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]))


def _inv(mp, A):
    d = _det(A)
    if d == 0:
        return None
    C = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            C[j, i] = (A[i1, j1] * A[i2, j2] - A[i1, j2] * A[i2, j1]) / d
    return C


def _eig(mp, S):
    E, Q = mp.eigsy(S)
    order = sorted(range(3), key=lambda c: E[c])
    return [E[c] for c in order], [[Q[r, c] for r in range(3)] for c in order]


def _chol(mp, S):
    L = mp.matrix(3, 3)
    for k in range(3):
        x = S[k, k] - sum(L[k, j] ** 2 for j in range(k))
        if not x > 0:
            return None
        L[k, k] = mp.sqrt(x)
        for i in range(k + 1, 3):
            L[i, k] = (S[i, k] - sum(L[i, j] * L[k, j] for j in range(k))) / L[k, k]
    return L


def build_exact(mp, case):
    nan = float("nan")
    out = dict(w=[nan] * 3, wu=[nan] * 3, inv=[nan] * 9, det=nan, chol=[nan] * 9, plane=[nan] * 4)
    cov = case["cov"]
    if not np.all(np.isfinite(cov)):
        return out
    A = _mat(mp, cov)
    w, vec = _eig(mp, _sym(mp, A, True))
    out["w"] = [float(x) for x in w]
    out["wu"] = [float(x) for x in _eig(mp, _sym(mp, A, False))[0]]
    out["det"] = float(_det(A))
    n = vec[0]
    nn = mp.sqrt(sum(x * x for x in n))
    big = max(range(3), key=lambda i: abs(n[i]))
    s = (1 if n[big] > 0 else -1) / nn
    n = [x * s for x in n]
    out["plane"] = [float(x) for x in n] + [float(sum(n[i] * mp.mpf(float(case["mean"][i])) for i in range(3)))]
    inv = _inv(mp, A)
    if inv is not None:
        out["inv"] = [float(inv[i, j]) for i in range(3) for j in range(3)]
        L = _chol(mp, _sym(mp, inv, True))
        if L is not None:
            out["chol"] = [float(L[i, j]) for i in range(3) for j in range(3)]
    return out


def graph_exact(mp, case):
    """GMMUtility::BHCoefficient (gmm_utils.h:30-52) for every ordered pair"""
    K = len(case["mean"])
    D = np.full((K, K), np.nan)
    cache = {}
    covs = [_mat(mp, case["cov"][i].reshape(3, 3)) for i in range(K)]
    dets = [_det(c) for c in covs]
    for i in range(K):
        for j in range(K):
            if i == j:
                continue
            dq = tuple(Fraction(float(case["mean"][j][a])) - Fraction(float(case["mean"][i][a])) for a in range(3))
            key = (case["cov"][i].tobytes(), case["cov"][j].tobytes(), dq)  # the distance depends on the exact difference only
            if key not in cache:
                dm = [mp.mpf(x.numerator) / mp.mpf(x.denominator) for x in dq]  # dyadic: exact at 60 digits
                S = (covs[i] + covs[j]) / 2
                inv = _inv(mp, S)
                pd = dets[i] * dets[j]
                val = float("nan")
                if inv is not None and pd > 0 and _det(S) > 0:
                    d0 = sum(dm[a] * inv[a, b] * dm[b] for a in range(3) for b in range(3)) / 8
                    d1 = mp.log(_det(S) / mp.sqrt(pd)) / 2
                    val = float(d0 + d1)
                cache[key] = val
            D[i, j] = cache[key]
    return D


def arrays():
    from tests import gmm_cases as gc
    mp = _mp()
    ex = [build_exact(mp, c) for c in gc.BUILD]
    out = {"build_" + k: np.array([e[k] for e in ex], dtype=np.float64) for k in ("w", "wu", "inv", "det", "chol", "plane")}
    for c in gc.GRAPH:
        out["graph_" + c["name"]] = graph_exact(mp, c)
    return out


def write(path):
    arrs = arrays()
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrs[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    write(sys.argv[1] if len(sys.argv) > 1 else DEFAULT)
