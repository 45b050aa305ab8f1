"""Hand-built cases for the map build (A0), the neighbour graph (A2) and the k-NN on the means (A6): one case on each side
of every decision, each with its name, the decision it targets, the side it lies on and its declared output.

Nothing here is random.  Means and covariances are literals, or R diag(w) R^T evaluated in rational arithmetic on the
binary values of w and rounded once per entry, so the inputs are the same bits on every machine.  The rotations are
rational and checked to be orthogonal in rationals at import.

The reference values are not the oracle's: tests/golden/gmm_cases_exact.npz (tools/make_gmm_cases_golden.py) holds,
from 60-digit arithmetic on the binary values of these inputs, the eigenvalues of the lower and of the upper triangle,
the inverse, the determinant, the Cholesky factor of the inverse's lower triangle, the plane (eigenvector of the
smallest eigenvalue and its offset) and every Bhattacharyya distance, each rounded to double at the end.

Decisions and the cases that hold them
  gaussian.cpp:44     w0 < 1e-4                       diag.at / diag.deg / rot.*       (strict: diag.at has w0 == 1e-4)
  gaussian.cpp:51-54  w1 > 0.2 && w2 > 0.2            diag.at / diag.sal / rot.*       (strict: diag.at has w1 == 0.2)
                      w2 > 0.2 alone decides nothing once the eigenvalues are sorted (w2 >= w1): no case can hold it
                      apart from the sort, which order.* hold.
  SelfAdjointView     lower triangle read             asym.* / asym2.*
  sort                ascending, columns move         order.*  (all six orders of three distinct entries)
  chol3_lower         !(x > 0) -> NaN                 bad.*
  gaussian_mixture.cpp:61-78  j != i, dist < thresh   GRAPH cases
  knnSearch           d < dist[k-1]; equal distances lowest index first (declared deviation from nanoflann's tree order)
"""
import math
from fractions import Fraction as Fr

import numpy as np

EPS = 2.0 ** -52
NAN, INF = float("nan"), float("inf")

# ---------------------------------------------------------------------------------------------------- rotations
_R1 = [[Fr(2, 3), Fr(-1, 3), Fr(2, 3)], [Fr(2, 3), Fr(2, 3), Fr(-1, 3)], [Fr(-1, 3), Fr(2, 3), Fr(2, 3)]]
_R2 = [[Fr(2, 7), Fr(3, 7), Fr(6, 7)], [Fr(3, 7), Fr(-6, 7), Fr(2, 7)], [Fr(6, 7), Fr(2, 7), Fr(-3, 7)]]  # not a permutation of R1
ROT = {"R1": _R1, "R2": _R2}
for _R in ROT.values():  # R R^T == I exactly
    assert all(sum(_R[i][k] * _R[j][k] for k in range(3)) == (1 if i == j else 0) for i in range(3) for j in range(3))


def rot_cov(R, w):
    """R diag(w) R^T in rationals on the binary values of w, each entry rounded once: symmetric, the same bits anywhere."""
    R = ROT[R]
    wq = [Fr(float(x)) for x in w]
    return np.array([[float(sum(R[i][k] * wq[k] * R[j][k] for k in range(3))) for j in range(3)] for i in range(3)])


def rot_col(R, c, scale=1.0):
    """scale * column c of the rotation, rounded once per entry"""
    return np.array([float(ROT[R][i][c] * Fr(float(scale))) for i in range(3)])


def diag(a, b, c):
    return np.diag([float(a), float(b), float(c)])


# ---------------------------------------------------------------------------------------------------- BUILD (A0)
# Each case: name, decision, side, mean, cov (3 x 3, row-major), declared flags (bit0 is_degenerated, bit1 is_salient),
# and what is declared about the decomposition:
#   axis   : the declared axis matrix itself (diagonal covariances: Jacobi performs no rotation)
#   normal_unique : the eigenvector of w0 is unique up to sign and is compared with the 60-digit plane; where it is
#            not, only n^T cov n = w0 is required
#   ok     : chol3_lower succeeds; where it does not, sqrt_info and hgw are NaN
#   thresh : (eigenvalue index, threshold) for the cases that sit next to a threshold: the CPU test requires the 60-digit
#            eigenvalue of the ROUNDED matrix on the declared side with >= 20x the oracle's own error as margin
BUILD = []
MEAN0 = (1.5, -2.25, 0.75)


def _b(name, decision, side, cov, flags, mean=MEAN0, axis=None, normal_unique=True, ok=True, thresh=()):
    BUILD.append(dict(name=name, decision=decision, side=side, mean=np.array(mean, dtype=np.float64),
                      cov=np.array(cov, dtype=np.float64), flags=flags, axis=axis, normal_unique=normal_unique, ok=ok,
                      thresh=tuple(thresh)))


W0T, W1T = 1e-4, 0.2
_below, _above = math.nextafter(W0T, 0.0), math.nextafter(W1T, 1.0)
# diagonal: the eigenvalues ARE the entries, so the strict comparisons are decidable exactly
_b("diag.at", "w0 < 1e-4, w1 > 0.2", "both equal: neither holds", diag(1.0, W0T, W1T), 0)
_b("diag.in", "w0 < 1e-4, w1 > 0.2", "one ulp inside both", diag(1.0, _below, _above), 3)
_b("diag.deg", "w0 < 1e-4", "one ulp below, w1 == 0.2", diag(1.0, _below, W1T), 1)
_b("diag.sal", "w1 > 0.2", "one ulp above, w0 == 1e-4", diag(1.0, W0T, _above), 2)
# all six orders of three distinct entries: the ascending sort, and the COLUMNS of axis moving with it.
# plane4 = (e_a, mean_a) with a = the position of the smallest entry.
_E = (5e-5, 0.5, 3.0)
for _p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
    _d = [_E[_p[0]], _E[_p[1]], _E[_p[2]]]  # entry at diagonal position i is the _p[i]-th smallest
    _ax = np.zeros((3, 3))
    for _i in range(3):
        _ax[_i, _p[_i]] = 1.0  # column c = e_(position of the c-th smallest)
    _b("order.%d%d%d" % _p, "sort ascending, columns with it", "entries in order %d%d%d" % _p, diag(*_d), 3, axis=_ax)
# rotated: w0 at 1e-4 (1 -+ 1e-6), w1 at 0.2 (1 +- 1e-6), under both rotations, three sizes of w2
for _R in ("R1", "R2"):
    for _w2 in (1.0, 50.0, 1e4):
        _b("rot.%s.%g.in" % (_R, _w2), "w0 < 1e-4, w1 > 0.2", "inside both by 1e-6 relative",
           rot_cov(_R, (W0T * (1 - 1e-6), W1T * (1 + 1e-6), _w2)), 3, thresh=((0, W0T), (1, W1T)))
        _b("rot.%s.%g.out" % (_R, _w2), "w0 < 1e-4, w1 > 0.2", "outside both by 1e-6 relative",
           rot_cov(_R, (W0T * (1 + 1e-6), W1T * (1 - 1e-6), _w2)), 0, thresh=((0, W0T), (1, W1T)))
# spectra
_b("iso", "spectrum", "isotropic: no eigenvector is unique", diag(0.3, 0.3, 0.3), 2, axis=np.eye(3), normal_unique=False)
_b("needle", "spectrum", "w0 == w1: the plane normal is not unique", rot_cov("R1", (5e-5, 5e-5, 2.0)), 1, normal_unique=False)
_b("disc", "spectrum", "w1 == w2", rot_cov("R2", (0.01, 0.5, 0.5)), 2)
_b("cond1e4", "spectrum", "oblique, condition 1e4", rot_cov("R2", (1e-3, 0.5, 10.0)), 2)
_b("cond1e6", "spectrum", "oblique, condition 1e6", rot_cov("R1", (1e-5, 0.5, 10.0)), 3)
_b("cond1e8", "spectrum", "oblique, condition 1e8", rot_cov("R2", (1e-7, 0.3, 10.0)), 3)
# asymmetric: the lower triangle has w0 = 5e-5, the upper one ~2e-4 (entry 01 raised by 1.6875e-4: dw0 = 2 v0 v1 e = 8e/9).
# saveGMMModel -> loadGMMModel transposes, so the loaded map reads the other triangle and gets the other flag.
_A = rot_cov("R1", (5e-5, 0.5, 3.0))
_A[0, 1] += 1.6875e-4
# The inverse of this matrix is asymmetric too, and the lower triangle chol3_lower reads is indefinite (-0.18 against entries
# of 3 556, a fact of the 60-digit values): as given the component has NaN sqrt_info and hgw; transposed it factorises.
_b("asym.lower", "which triangle eig_sym reads", "as given: lower triangle, w0 = 5e-5", _A, 3, ok=False, thresh=((0, W0T),))
_b("asym.saved", "which triangle eig_sym reads", "after save -> load (transposed): w0 ~ 2e-4", _A.T.copy(), 2, thresh=((0, W0T),))
# the same with 8e-5 below and ~1.2e-4 above (entry 01 raised by 4.5e-5): both orientations factorise
_A2 = rot_cov("R1", (8e-5, 0.5, 3.0))
_A2[0, 1] += 4.5e-5
_b("asym2.lower", "which triangle eig_sym reads", "as given: lower triangle, w0 = 8e-5", _A2, 3, thresh=((0, W0T),))
_b("asym2.saved", "which triangle eig_sym reads", "after save -> load (transposed): w0 ~ 1.2e-4", _A2.T.copy(), 2, thresh=((0, W0T),))
# chol3_lower fails: sqrt_info and hgw are NaN, flags as declared (selection sort with `<`, NaN compares false)
_b("bad.indef", "chol3_lower !(x > 0)", "indefinite", diag(1.0, -0.5, 2.0), 3, ok=False,
   axis=np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, 1]]))
_b("bad.singular", "chol3_lower !(x > 0)", "singular: 1/det = inf", diag(1.0, 0.0, 2.0), 3, ok=False,
   axis=np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, 1]]))
_b("bad.inf", "chol3_lower !(x > 0)", "an infinite entry: sorted last, w1 = 2", diag(1.0, INF, 2.0), 2, ok=False,
   axis=np.array([[1.0, 0, 0], [0, 0, 1], [0, 1, 0]]))
_b("bad.nan", "chol3_lower !(x > 0)", "a NaN entry: never moves in the sort, w1 = NaN is not > 0.2", diag(1.0, NAN, 2.0), 0,
   ok=False, axis=np.eye(3))
BUILD_BY_NAME = {c["name"]: c for c in BUILD}
BUILD_K_EDGES = (1, 127, 128, 129)  # the block edge of k_build_components, the decisive case (diag.in) in the last slot


def build_map(names):
    cs = [BUILD_BY_NAME[n] for n in names]
    return np.stack([c["mean"] for c in cs]), np.stack([c["cov"].reshape(9) for c in cs])


def build_edge_map(K, last="diag.in"):
    """K - 1 plain components (identity covariance: flags 2) and the decisive case in the last slot"""
    mean = np.array([[float(i), 0.0, 0.0] for i in range(K)])
    cov = np.tile(np.eye(3).reshape(9), (K, 1))
    c = BUILD_BY_NAME[last]
    mean[K - 1], cov[K - 1] = c["mean"], c["cov"].reshape(9)
    return mean, cov, np.array([2] * (K - 1) + [c["flags"]], dtype=np.uint8)


def flags_of(w, deg=lambda a, b: a < b, sal=lambda a, b: a > b):
    """gaussian.cpp:44,51-54 on given eigenvalues; the comparisons are arguments so a test can alter one"""
    return (1 if deg(w[0], W0T) else 0) | (2 if (sal(w[1], W1T) and sal(w[2], W1T)) else 0)


def hgw_of(L):
    """J^T J of EdgePt2Gaussian = L L^T (00 01 02 11 12 22) in k_build_components' expression order, from (n, 9) sqrt_info"""
    L = L.reshape(-1, 3, 3)
    return np.stack([(L[:, i, 0] * L[:, j, 0] + L[:, i, 1] * L[:, j, 1]) + L[:, i, 2] * L[:, j, 2]
                     for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)


def plane4_of(axis, mean):
    """EdgePt2GaussianDeg's plane in k_build_components' expression order, from (n, 9) axis and (n, 3) mean"""
    n = axis.reshape(-1, 3, 3)[:, :, 0]
    return np.concatenate([n, ((n[:, 0] * mean[:, 0] + n[:, 1] * mean[:, 1]) + n[:, 2] * mean[:, 2])[:, None]], axis=1)


# ---------------------------------------------------------------------------------------------------- GRAPH (A2)
# Each case: name, decision, side, mean (K x 3), cov (K x 9), thresh, rows = the declared neighbour list of every component.
GRAPH = []
I3 = np.eye(3).reshape(9)


def _g(name, decision, side, mean, cov, rows, thresh=2.5):
    mean, cov = np.array(mean, dtype=np.float64).reshape(-1, 3), np.array(cov, dtype=np.float64).reshape(-1, 9)
    assert len(mean) == len(cov) == len(rows)
    GRAPH.append(dict(name=name, decision=decision, side=side, mean=mean, cov=cov, thresh=thresh, rows=[list(r) for r in rows]))


_PAIR, _NONE = [[1], [0]], [[], []]
# equal isotropic: dist = d^2 / (8 sigma^2), log term 0.  d = sqrt(20 (1 -+ 1e-6)) as a literal.
_g("thr.iso.in", "dist < thresh", "2.5 (1 - 1e-6)", [[0, 0, 0], [4.472133718931043, 0, 0]], [I3, I3], _PAIR)
_g("thr.iso.out", "dist < thresh", "2.5 (1 + 1e-6)", [[0, 0, 0], [4.472138191066998, 0, 0]], [I3, I3], _NONE)
# unequal isotropic (1 and 4): log term 1/2 ln(2.5^3 / 8) = 0.33472..., d^2 / 20 makes up the rest
_g("thr.uneq.in", "dist < thresh", "2.5 (1 - 1e-6), log term 0.335", [[0, 0, 0], [0, 6.580702353136306, 0]], [I3, 4 * I3], _PAIR)
_g("thr.uneq.out", "dist < thresh", "2.5 (1 + 1e-6), log term 0.335", [[0, 0, 0], [0, 6.580709951105102, 0]], [I3, 4 * I3], _NONE)
# a pair of oblique discs R2 diag(0.01, 0.5, 0.5) R2^T, offset t along the thin axis: dist = t^2 / 0.08
_DISC = rot_cov("R2", (0.01, 0.5, 0.5)).reshape(9)
_g("thr.disc.in", "dist < thresh", "2.5 (1 - 1e-6), oblique discs", [MEAN0, np.array(MEAN0) + rot_col("R2", 0, 0.4472133718931043)],
   [_DISC, _DISC], _PAIR)
_g("thr.disc.out", "dist < thresh", "2.5 (1 + 1e-6), oblique discs", [MEAN0, np.array(MEAN0) + rot_col("R2", 0, 0.4472138191066998)],
   [_DISC, _DISC], _NONE)
# a non-default threshold through params: 1.0, d = sqrt(8 (1 -+ 1e-6))
_g("thr.param.in", "neighbor_dist_thresh from params", "1.0 (1 - 1e-6)", [[0, 0, 0], [0, 0, 2.828425710532274]], [I3, I3], _PAIR, 1.0)
_g("thr.param.out", "neighbor_dist_thresh from params", "1.0 (1 + 1e-6)", [[0, 0, 0], [0, 0, 2.8284285389593986]], [I3, I3], _NONE, 1.0)
_g("thr.param.default", "neighbor_dist_thresh from params", "the same pair under 2.5", [[0, 0, 0], [0, 0, 2.8284285389593986]],
   [I3, I3], _PAIR)
# structure
_g("k1", "j != i", "one component: nnz = 0", [[0, 0, 0]], [I3], [[]])
_g("k2.same", "j != i; duplicates are neighbours (the reference compares pointers)", "two equal components, dist 0",
   [MEAN0, MEAN0], [_DISC, _DISC], _PAIR)
for _K in (63, 64, 65, 129):  # on a line, spacing 4: dist 2 to i +- 1, 8 to i +- 2
    _g("line.%d" % _K, "dist < thresh; row order; K mod 4 = %d" % (_K % 4), "only i +- 1",
       [[4.0 * i, 0, 0] for i in range(_K)], [I3] * _K, [[j for j in (i - 1, i + 1) if 0 <= j < _K] for i in range(_K)])
_g("complete.130", "j != i; ballot prefix carried over three 64-lane chunks", "130 coincident components: every row all but i",
   [[0.5, 0.25, -1.0]] * 130, [0.3 * I3] * 130, [[j for j in range(130) if j != i] for i in range(130)])
# 70 components 100 apart, the last one on top of component 5: its row's only entry is K - 1, in the partial second chunk
_g("last.70", "partial chunk; K mod 4 = 2", "row 5 = [69], row 69 = [5]",
   [[100.0 * i, 0, 0] for i in range(69)] + [[500.0, 0, 0]], [I3] * 70,
   [([69] if i == 5 else [5] if i == 69 else []) for i in range(70)])
# dist == thresh exactly: (4, 0, 0) apart under the identity is 16 / 8 = 2.0 with no rounding anywhere (the inverse of I, log 1)
_g("thr.equal", "dist < thresh is strict", "dist == thresh == 2.0: not a neighbour", [[0, 0, 0], [4, 0, 0]], [I3, I3], _NONE, 2.0)
_g("k3.mod3", "K mod 4 = 3", "three coincident", [[1, 2, 3]] * 3, [I3] * 3, [[1, 2], [0, 2], [0, 1]])
# one component with det < 0 between coincident ones: sqrt(det_i det_j) is NaN, so it has no row and is in no row
_g("negdet", "dist < thresh with dist = NaN", "component 1 has det = -1", [[0, 0, 0]] * 3, [I3, diag(1, -1, 1).reshape(9), I3],
   [[2], [], [0]])
# three oblique components of different shape (one of condition 1e6): the distances 1.98, 1.51 and 4.02 are far from the
# threshold; this case is here for the value of nbs_dist, which every rounding of the formula touches
_g("oblique.3", "value of nbs_dist", "0-1 and 0-2 neighbours, 1-2 not",
   [MEAN0, np.array(MEAN0) + np.array([0.3, -0.2, 0.1]), np.array(MEAN0) + np.array([-0.05, 0.1, 0.2])],
   [rot_cov("R1", (0.01, 0.5, 3.0)).reshape(9), rot_cov("R2", (0.02, 0.3, 5.0)).reshape(9), rot_cov("R1", (1e-5, 0.5, 10.0)).reshape(9)],
   [[1, 2], [0], [0]])
GRAPH_BY_NAME = {c["name"]: c for c in GRAPH}


def load_exact():
    """tests/golden/gmm_cases_exact.npz -> ([per BUILD case dict(w, wu, inv, det, chol, plane)], {GRAPH name: K x K distances})"""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmm_cases_exact.npz"))
    build = [{k: d["build_" + k][i] for k in ("w", "wu", "inv", "det", "chol", "plane")} for i in range(len(BUILD))]
    return build, {c["name"]: d["graph_" + c["name"]] for c in GRAPH}


def csr_of(rows):
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, np.array([j for r in rows for j in r], dtype=np.int32)


def graph_rule(dist, thresh, lt=lambda a, b: a < b, skip_self=True):
    """gaussian_mixture.cpp:61-78 on a K x K distance matrix; the comparison and `j != i` are arguments"""
    K = dist.shape[0]
    return [[j for j in range(K) if not (skip_self and j == i) and lt(dist[i, j], thresh)] for i in range(K)]


# ---------------------------------------------------------------------------------------------------- KNN (A6)
# Integer lattice means (filler queries are dyadic), so every squared distance is exact in double.
# Each case: name, decision, side, mean (K x 3), q (the decisive query), want = {k: declared index list}; the lists not
# written by hand follow knn_rule, and the hand-written ones hold knn_rule.
KNN = []
FILLER_Q = (0.5, -0.25, 0.125)  # the other queries of a batch


def knn_rule(mean, q, k, before=lambda a, b: a < b, accept=lambda a, b: a < b):
    """The declared rule: the k smallest squared distances, ascending, equal distances lowest index first, padded with
    (-1, +inf).  Written as the insertion the kernels perform: `accept` gates an entry against the current k-th, `before`
    places it; both are arguments so a test can alter one."""
    idx, dist = [-1] * k, [INF] * k
    for g in range(len(mean)):
        d0, d1, d2 = q[0] - mean[g][0], q[1] - mean[g][1], q[2] - mean[g][2]
        d = (d0 * d0 + d1 * d1) + d2 * d2
        if accept(d, dist[k - 1]):
            i = 0
            while i < k and not before(d, dist[i]):
                i += 1
            if i < k:
                idx[i + 1:], dist[i + 1:] = idx[i:k - 1], dist[i:k - 1]
                idx[i], dist[i] = g, d
    return idx, dist


def _k(name, decision, side, mean, q=(0.0, 0.0, 0.0), want=None, ks=tuple(range(1, 9))):
    mean = np.array(mean, dtype=np.float64).reshape(-1, 3)
    w = {k: knn_rule(mean, q, k)[0] for k in ks}
    for k, v in (want or {}).items():
        assert w[k] == list(v), (name, k, w[k], v)  # the hand-written lists hold the rule
    KNN.append(dict(name=name, decision=decision, side=side, mean=mean, q=np.array(q, dtype=np.float64), want=w,
                    hand=sorted((want or {}).keys())))


def _far(K):
    return [[1000.0 + i, 0.0, 0.0] for i in range(K)]


def _with(K, near):
    m = _far(K)
    for i, p in near.items():
        m[i] = [float(x) for x in p]
    return m


# +-e_x, +-e_y, +-e_z, 2e_x, 2e_y, then copies of the first three: nine means at distance 1, so a tie straddles every k <= 8.
# Observed from the reference's own nanoflann on this map (tree order): k = 1 -> [9], k = 3 -> [9 1 5],
# k = 8 -> [9 1 5 3 4 2 10 8].
_OCTA = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [2, 0, 0], [0, 2, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0]]
NANOFLANN_OCTA = {1: [9], 3: [9, 1, 5], 8: [9, 1, 5, 3, 4, 2, 10, 8]}
_k("tie.straddle", "equal distances: lowest index first", "nine at distance 1: the tie straddles the k-th place for every k",
   _OCTA, want={1: [0], 3: [0, 1, 2], 8: [0, 1, 2, 3, 4, 5, 8, 9]})
_k("tie.inside", "equal distances: lowest index first", "three at distance 1 inside the first k (k >= 3), all else distinct",
   [[2, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 0], [0, 4, 0], [0, 0, 5], [6, 0, 0], [0, 7, 0], [0, 0, 8]],
   want={1: [1], 2: [1, 2], 3: [1, 2, 3], 4: [1, 2, 3, 0], 8: [1, 2, 3, 0, 4, 5, 6, 7]})
_k("dup.lanes", "equal distances: lowest index first", "duplicates on one lane (3, 67) and on others (10, 131)",
   _with(132, {3: (1, 0, 0), 67: (1, 0, 0), 10: (0, 1, 0), 131: (0, 0, 1)}),
   want={1: [3], 2: [3, 10], 3: [3, 10, 67], 4: [3, 10, 67, 131], 5: [3, 10, 67, 131, 0]})
for _K in (1, 3, 7, 8, 9):  # fewer means than k: padded with (-1, +inf)
    _k("pad.%d" % _K, "K < k: padding", "K = %d under k = 5 and k = 8" % _K, [[i + 1, 0, 0] for i in range(_K)],
       want={5: (list(range(_K)) + [-1] * 5)[:5], 8: (list(range(_K)) + [-1] * 8)[:8]})
for _K in (63, 64, 65):  # lanes of the wave kernel: the nearest is the last index
    _k("lane.%d" % _K, "wave kernel lanes", "nearest at K - 1 = %d, then descending" % (_K - 1),
       [[_K - i, 0, 0] for i in range(_K)], want={3: [_K - 1, _K - 2, _K - 3]})
# the 512-mean LDS tile of the thread kernel
_k("tile.511", "LDS tile edge", "K = 511: the winner in the last slot of a partial tile", _with(511, {510: (1, 0, 0), 7: (2, 0, 0)}),
   want={2: [510, 7]})
_k("tile.512", "LDS tile edge", "K = 512: the winner at 511, the last slot of a full tile", _with(512, {511: (1, 0, 0), 0: (2, 0, 0)}),
   want={2: [511, 0]})
_k("tile.513", "LDS tile edge", "K = 513: the winner at 512 alone in the second tile, 511 and 512 tie with 3",
   _with(513, {512: (1, 0, 0), 511: (0, 1, 0), 3: (0, 0, 1), 510: (2, 0, 0)}), want={1: [3], 3: [3, 511, 512], 4: [3, 511, 512, 510]})
_k("tile.513w", "LDS tile edge", "K = 513: the only near mean is 512, alone in the second tile", _with(513, {512: (1, 0, 0), 0: (2, 0, 0)}),
   want={1: [512], 2: [512, 0]})
_k("tile.1025", "LDS tile edge", "K = 1025: the winner at 1024 in a tile of one, the k nearest split over three tiles",
   _with(1025, {1024: (1, 0, 0), 512: (2, 0, 0), 511: (3, 0, 0), 1023: (4, 0, 0), 0: (5, 0, 0)}),
   want={1: [1024], 5: [1024, 512, 511, 1023, 0]})
_k("nan.query", "d < dist[k-1] with d = NaN", "a NaN query: nothing is ever accepted", [[1, 0, 0], [2, 0, 0], [3, 0, 0]],
   q=(NAN, 0.0, 0.0), want={5: [-1] * 5, 8: [-1] * 8})
_k("nan.mean", "d < dist[k-1] with d = NaN", "a NaN mean is never returned", [[2, 0, 0], [NAN, 0, 0], [1, 0, 0], [0, 3, 0]],
   want={1: [2], 5: [2, 0, 3, -1, -1]})
KNN_BY_NAME = {c["name"]: c for c in KNN}
KNN_POSITIONS = (0, 255, 256, -1)  # where the decisive query goes in a thread-kernel batch (first, block edge, last)
KNN_WAVE_N = (1, 3, 4, 5)          # N that select the wave kernel (a block holds four queries)


def knn_batch(case, N):
    """(N, 3) queries: FILLER_Q everywhere, the decisive query at KNN_POSITIONS (where N has them) -> (queries, decisive mask)"""
    q = np.tile(np.array(FILLER_Q), (N, 1))
    dec = np.zeros(N, bool)
    for p in KNN_POSITIONS:
        if -N <= p < N:
            dec[p] = True
    q[dec] = case["q"]
    return q, dec


def knn_expected(case, N, k):
    """declared (idx, dist) of knn_batch(case, N)"""
    q, dec = knn_batch(case, N)
    a = knn_rule(case["mean"], case["q"], k)
    b = knn_rule(case["mean"], FILLER_Q, k)
    assert a[0] == case["want"][k]
    idx = np.where(dec[:, None], np.array(a[0], np.int32), np.array(b[0], np.int32)).astype(np.int32)
    dist = np.where(dec[:, None], np.array(a[1]), np.array(b[1]))
    return q, idx, dist


# ---------------------------------------------------------------------------------------------------- bounds
# Error of the CPU oracle against the 60-digit values, worst over every case above, measured by
# tests/test_gmm_cases.py::test_oracle_error_figures (which asserts them from above).  Units:
#   scale      |w - w_exact|                                    eps * w2
#   residual   max_c ||cov v_c - w_c v_c||_inf                  eps * w2      (evaluated in long double)
#   ortho      max |V^T V - I|                                  eps
#   normal     |n^T cov n - w0|  (also the non-unique normals)  eps * w2
#   plane_n    max |n - n_exact| up to sign (unique normals)    eps * w2 / (w1 - w0)
#   plane_d    |offset - offset_exact|, same sign               eps * w2 / (w1 - w0) * ||mean||_1
#   hgw        max |hgw - inverse_exact|                        eps * kappa * max |inverse_exact|
#   sqrt_info  max |L - chol(inverse_exact)|                    eps * kappa * max |L_exact|
#   nbs_dist   |dist - dist_exact|                              eps * kappa * max(1, |dist_exact|), the pair's larger kappa
# kappa = (w2 / w0) (w2 / w1) is the amplification of the cofactor inverse the reference uses (Eigen's 3 x 3 inverse): the
# cofactors carry an absolute error of eps w2^2, and the determinant w0 w1 w2 is their sum against entries of size w2.
# The device runs the same expression order with -ffp-contract=off, so it may differ from the oracle by the rounding of
# sqrt and division alone: it gets 4x the oracle's worst figure with a floor of 8 units.
ORACLE_WORST = {  # measured figure (the case it came from), rounded up to two digits
    "scale": 2.0,        # 1.92   rot.R2.50.in
    "residual": 1.8,     # 1.72   rot.R2.50.in
    "ortho": 4.2,        # 4.17   rot.R1.10000.out
    "normal": 0.016,     # 0.0155 disc
    "plane_n": 0.5,      # 0.49   disc
    "plane_d": 0.12,     # 0.111  rot.R1.1.out
    "hgw": 0.043,        # 0.042  rot.R1.1.out
    "sqrt_info": 0.043,  # 0.0422 disc
    "nbs_dist": 0.0019,  # 0.00184 oblique.3; every other GRAPH case is exact to the last bit
}
DEVICE_BOUND = {q: max(4.0 * v, 8.0) for q, v in ORACLE_WORST.items()}


def kappa(w):
    return (w[2] / w[0]) * (w[2] / w[1])


def build_errors(got, ex, case):
    """Errors of one built component in the units above.  got: dict(scale (3,), axis (9,), sqrt_info (9,), hgw (6,),
    plane4 (4,)); ex: the component's 60-digit values dict(w, inv, chol, plane).  Quantities that do not apply are absent."""
    out = {}
    ld = np.longdouble
    cov = case["cov"]
    low = np.tril(cov) + np.tril(cov, -1).T  # the matrix eig_sym decomposes
    w_ex = ex["w"]
    if not np.all(np.isfinite(cov)):
        return out
    w2 = max(abs(w_ex[0]), abs(w_ex[2]))
    u = EPS * w2
    V = got["axis"].reshape(3, 3)
    out["scale"] = np.abs(got["scale"] - w_ex).max() / u
    r = low.astype(ld) @ V.astype(ld) - V.astype(ld) * got["scale"].astype(ld)[None, :]
    out["residual"] = float(np.abs(r).max()) / u
    out["ortho"] = float(np.abs(V.astype(ld).T @ V.astype(ld) - np.eye(3)).max()) / EPS
    n = V[:, 0].astype(ld)
    out["normal"] = float(abs(n @ low.astype(ld) @ n - ld(w_ex[0]))) / u
    if case["normal_unique"]:
        gap = w_ex[1] - w_ex[0]
        s = 1.0 if float(np.dot(V[:, 0], ex["plane"][:3])) >= 0 else -1.0
        out["plane_n"] = np.abs(got["plane4"][:3] - s * ex["plane"][:3]).max() / (u / gap)
        out["plane_d"] = abs(got["plane4"][3] - s * ex["plane"][3]) / (u / gap * np.abs(case["mean"]).sum())
    if case["ok"]:
        cond = kappa(w_ex)
        inv = ex["inv"].reshape(3, 3)
        inv_low = np.array([inv[0, 0], inv[1, 0], inv[2, 0], inv[1, 1], inv[2, 1], inv[2, 2]])  # chol3_lower reads the lower triangle
        out["hgw"] = np.abs(got["hgw"] - inv_low).max() / (EPS * cond * np.abs(ex["inv"]).max())
        out["sqrt_info"] = np.abs(got["sqrt_info"] - ex["chol"]).max() / (EPS * cond * np.abs(ex["chol"]).max())
    return out


def graph_dist_errors(ptr, col, dist, dist_ex, cond):
    """errors of a CSR's distances in units eps * kappa * max(1, |dist_exact|) (cond: (K,) kappa per component)"""
    out = []
    for i in range(len(ptr) - 1):
        for e in range(ptr[i], ptr[i + 1]):
            j = col[e]
            out.append(abs(dist[e] - dist_ex[i, j]) / (EPS * max(cond[i], cond[j]) * max(1.0, abs(dist_ex[i, j]))))
    return max(out) if out else 0.0


# ---------------------------------------------------------------------------------------------------- shared checks
ALL_BUILD = [c["name"] for c in BUILD]


def check_build(got, exact_build, names, where):
    """the declared outputs of the BUILD cases `names` (row i of `got` = case names[i]); returns the worst error per quantity"""
    worst = {}
    for i, n in enumerate(names):
        c, ex = BUILD_BY_NAME[n], exact_build[[b["name"] for b in BUILD].index(n)]
        assert got["flags"][i] == c["flags"], (where, n, got["flags"][i])
        if c["axis"] is not None:  # diagonal covariance: no rotation, the sorted columns themselves
            assert np.array_equal(got["axis"][i].reshape(3, 3), c["axis"]), (where, n)
            a = int(np.argmax(c["axis"][:, 0]))
            assert np.array_equal(got["plane4"][i], np.concatenate([c["axis"][:, 0], [c["mean"][a]]])), (where, n)
        if c["axis"] is not None and np.all(np.isfinite(c["cov"])):
            assert np.array_equal(got["scale"][i], np.sort(np.diag(c["cov"]))), (where, n)  # the entries, exactly
        if not c["ok"]:
            assert np.isnan(got["sqrt_info"][i]).all() and np.isnan(got["hgw"][i]).all(), (where, n)
        else:
            assert np.isfinite(got["sqrt_info"][i]).all() and np.isfinite(got["hgw"][i]).all(), (where, n)
        e = build_errors({k: got[k][i] for k in ("scale", "axis", "sqrt_info", "hgw", "plane4")}, ex, c)
        for q, v in e.items():
            if v > worst.get(q, (-1.0, ""))[0]:
                worst[q] = (float(v), n)
    return worst


def check_graph(c, ptr, col, dist, dist_ex, cond):
    """declared rows, symmetry with equal bits, and the error of the distances in gmm_cases' units"""
    wptr, wcol = csr_of(c["rows"])
    assert np.array_equal(ptr, wptr) and np.array_equal(col, wcol), c["name"]
    d = {}
    for i in range(len(ptr) - 1):
        for e in range(ptr[i], ptr[i + 1]):
            d[(i, int(col[e]))] = dist[e]
    for (i, j), v in d.items():
        assert (j, i) in d and d[(j, i)].tobytes() == v.tobytes(), (c["name"], i, j)
    return graph_dist_errors(ptr, col, dist, dist_ex, cond)


def graph_cond(c):
    """kappa per component from LAPACK's eigenvalues (a unit, not a reference); 1 where the covariance is not positive definite"""
    w = np.linalg.eigvalsh(c["cov"].reshape(-1, 3, 3))
    return np.array([kappa(x) if x[0] > 0 else 1.0 for x in w])
