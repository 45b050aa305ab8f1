"""A bit-exact host model of the association arithmetic, in pure Python.  Test infrastructure for tests/assoc_cases.py,
tests/test_assoc_cases.py (CPU) and tests/test_gpu_assoc_cases.py.

A Python float is an IEEE double and +, -, *, / and math.sqrt round correctly, so an expression written in the source's order gives the
source's bits as long as the compiler does not contract (the library is built with -ffp-contract=off).  The one operation Python lacks
before 3.13, the fused multiply-add, goes through fractions.Fraction: float(Fraction) rounds correctly.

  record(mean, cov)          the 12 doubles k_build_components stores: mean[3], inv3(cov)[9] (gl_gmm.hip, gl_device.hpp)
  chi2_device(record, p)     chi2_rec / chi2_srec (gl_device.hpp): what every association path evaluates for a pair
  chi2_exact(cov, mean, p)   (p - mean)^T cov^-1 (p - mean) of the same doubles in rational arithmetic: the high-precision reference
  admitted(mean, cov)        the host predicate of build_cell_index (gl_grid.hip): does the component get lists in the grid, or is it
                             one of the `always` components every point evaluates
  gate_error_bound(w)        the bound of gl_grid.hip on |computed / exact - 1| of chi2, from the eigenvalues
  registered_gate(cov)       the chi2 (over 9) at which an admitted component is registered; slack_of(cov): what that leaves for the error
  source_constants()         the margins, read from gl_grid.hip itself
  grid_lo(mean, cov)         the origin of the grid; box_last_cell(...): the last cell of a component's box along an axis
"""
import math
import os
import re
from fractions import Fraction as Fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_SRC = os.path.join(ROOT, "gmmloc_amd", "csrc", "gl_grid.hip")
T_GATE = 9.0
U = 2.0 ** -53


def fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fr(a) * Fr(b) + Fr(c))


# ---- gl_device.hpp ---------------------------------------------------------------------------------------------------------------------
def cof3(m, i, j):
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1]


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:  # IEEE: 1 / +-0 = +-inf, 0 / 0 = nan
        return math.nan if a == 0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def inv3(m):
    c0, c1, c2 = cof3(m, 0, 0), cof3(m, 1, 0), cof3(m, 2, 0)
    det = (c0 * m[0] + c1 * m[3]) + c2 * m[6]
    invdet = _div(1.0, det)
    return [c0 * invdet, c1 * invdet, c2 * invdet,
            cof3(m, 0, 1) * invdet, cof3(m, 1, 1) * invdet, cof3(m, 2, 1) * invdet,
            cof3(m, 0, 2) * invdet, cof3(m, 1, 2) * invdet, cof3(m, 2, 2) * invdet]


def det3(m):
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])


def _flat(a, n):
    out = [float(x) for row in a for x in (row if hasattr(row, "__len__") else [row])]
    assert len(out) == n
    return out


def record(mean, cov):
    return _flat(mean, 3) + inv3(_flat(cov, 9))


def chi2_device(rec, p):
    x, y, z = (float(v) for v in p)
    d0, d1, d2 = x - rec[0], y - rec[1], z - rec[2]
    r0 = fma(d2, rec[9], fma(d1, rec[6], d0 * rec[3]))
    r1 = fma(d2, rec[10], fma(d1, rec[7], d0 * rec[4]))
    r2 = fma(d2, rec[11], fma(d1, rec[8], d0 * rec[5]))
    return fma(r2, d2, fma(r1, d1, r0 * d0))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def chi2_exact(cov, mean, p):
    """Fraction: d^T cov^-1 d with d = p - mean, everything exact (adjugate over determinant)"""
    m = [Fr(v) for v in _flat(cov, 9)]
    d = [Fr(float(a)) - Fr(float(b)) for a, b in zip(p, _flat(mean, 3))]

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1]
    det = m[0] * cof(0, 0) + m[1] * cof(0, 1) + m[2] * cof(0, 2)
    # inverse[i][j] = cof(j, i) / det
    return sum(d[i] * cof(j, i) * d[j] for i in range(3) for j in range(3)) / det


# ---- gl_grid.hip: the host side of build_cell_index ---------------------------------------------------------------------------------------
def eig3_sym(c):
    """eigenvalues of a symmetric 3x3 by cyclic Jacobi, ascending: eig3_sym of gl_grid.hip, operation for operation"""
    a = [[c[0], c[1], c[2]], [c[1], c[4], c[5]], [c[2], c[5], c[8]]]
    for _ in range(30):
        off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2]
        if off < 1e-300:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if a[p][q] == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                cs = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * cs
                for k in range(3):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p] = cs * akp - sn * akq
                    a[k][q] = sn * akp + cs * akq
                for k in range(3):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k] = cs * apk - sn * aqk
                    a[q][k] = sn * apk + cs * aqk
    return sorted([a[0][0], a[1][1], a[2][2]])


_constants = None


def source_constants():
    """the margins build_cell_index uses, read from its source: dict(reg, resolve, cell_eps, cond, asym, err_pair, err_one, err_max, slack)"""
    global _constants
    if _constants is None:
        src = open(GRID_SRC).read()

        def one(pat):
            m = re.findall(pat, src)
            assert len(m) == 1, (pat, m)
            return float(m[0])
        num = r"([0-9.]+(?:e[+-]?[0-9]+)?)"
        c = dict(reg=one(r"t_reg = T \* \(1\.0 \+ " + num + r"\)"), resolve=one(r"t_resolve = T \* \(1\.0 \+ " + num + r"\)"),
                 cell_eps=one(r"in = in && \(q <= 1\.0 \+ " + num + r"\)"), asym=one(r"asym > " + num + r" \* w\[2\]"),
                 cond=one(r"kCondMax = " + num + ";"), err_pair=one(r"kErrPair = " + num + ";"), err_one=one(r"kErrOne = " + num + ";"),
                 err_max=one(r"kErrMax = " + num + ";"))
        # What the source leaves for the error of the computed chi2: a point resolved at computed chi2 <= T (1 + resolve) must lie inside
        # the registered ellipsoid T (1 + reg).  The 1e-9 inflations (ext, the forms' <= 1 + 1e-9, rho) pay for the registration's own
        # rounding and are not available twice: one of them in length is two in chi2.
        c["slack"] = (1.0 + c["reg"]) / (1.0 + c["resolve"]) - 1.0 - 2.0 * c["cell_eps"]
        # the gate of its own of a component whose bound exceeds the slack: the statement itself, and that semi-axes, box and the
        # three bounding forms are made from it
        c["widen"] = len(re.findall(r"if \(err > slack\) treg\[k\] = t_reg / \(1\.0 - err\);", src)) == 1
        uses = (r"const double t_k = treg\[k\];", r"std::sqrt\(t_k \* w\[a\]\)", r"std::sqrt\(t_k \* cv\[a \* 4\]\)", r"\(1\.0 \+ 1\.0 / betas\[b\]\) \* treg\[k\]")
        c["widen_used"] = all(len(re.findall(u, src)) == 1 for u in uses)
        _constants = c
    return _constants


def gate_error_bound(w):
    """build_cell_index's first-order bound on |computed chi2 / exact chi2 - 1| from the ascending eigenvalues (head of gl_grid.hip)"""
    c = source_constants()
    return U * (c["err_pair"] * (w[2] / w[0]) * (w[2] / w[1]) + c["err_one"] * (w[2] / w[0]))


def admitted(mean, cov):
    """True: the component is registered in the grid.  False: it is on the global list (`always`).  None: non-finite, it is on neither
    (its chi2 is NaN for every point).  The box limit (assoc_globcells) depends on the grid and is not part of this predicate."""
    c = source_constants()
    cv, mu = _flat(cov, 9), _flat(mean, 3)
    if not all(math.isfinite(v) for v in cv + mu):
        return None
    w = eig3_sym(cv)
    asym = abs(cv[1] - cv[3]) + abs(cv[2] - cv[6]) + abs(cv[5] - cv[7])
    if not (w[0] > 0.0) or not (w[2] / w[0] <= c["cond"]) or asym > c["asym"] * w[2]:
        return False
    return gate_error_bound(w) <= c["err_max"]


def registered_gate(cov):
    """the chi2 at which build_cell_index registers an admitted component, over T: 1 + reg, or (1 + reg) / (1 - err) where the bound
    exceeds the slack - if the source has that statement and uses its result"""
    c = source_constants()
    err = gate_error_bound(eig3_sym(_flat(cov, 9)))
    return (1.0 + c["reg"]) / (1.0 - err) if err > c["slack"] and c["widen"] and c["widen_used"] else 1.0 + c["reg"]


def slack_of(cov):
    """what the registration of this admitted component leaves for the error of its computed chi2 at the gate"""
    c = source_constants()
    return registered_gate(cov) / (1.0 + c["resolve"]) - 1.0 - 2.0 * c["cell_eps"]


def box_ext(cov, a, gate):
    """half the side of a component's registered box along axis a, for a registration gate given over T"""
    return math.sqrt(T_GATE * gate * _flat(cov, 9)[a * 4]) * (1.0 + 1e-9)


def grid_lo(mean, cov):
    """the origin of the grid build_cell_index lays over a map: the low corner of the registered boxes of the admitted components, less
    1e-6 of the span and 1e-9"""
    lo, hi = [1e300] * 3, [-1e300] * 3
    for m, cv in zip(mean, cov):
        if admitted(m, cv) is not True:
            continue
        g = registered_gate(cv)
        for a in range(3):
            e = box_ext(cv, a, g)
            lo[a], hi[a] = min(lo[a], float(m[a]) - e), max(hi[a], float(m[a]) + e)
    return [lo[a] - (1e-6 * (hi[a] - lo[a]) + 1e-9) for a in range(3)]


def box_last_cell(mu_a, ext, lo_a, h):
    """i1 of build_cell_index: the last cell along an axis that a box reaching mu_a + ext overlaps"""
    return math.floor((mu_a + ext - lo_a) / h + 1e-9)
