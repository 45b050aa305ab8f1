"""Hand-built maps and points on both sides of every decision of the exact cell index (gmmloc_amd/csrc/gl_grid.hip), for
tests/test_assoc_cases.py (CPU: the bit-exact model of tests/assoc_model.py against rational arithmetic) and
tests/test_gpu_assoc_cases.py (every case through the index, both sweeps, the oracle and gl_track_frames).  Test infrastructure.

A random cloud almost never puts a point where the index's argument is thin: within 1e-5 of a component's chi2 = 9 surface, at the
tips of its longest axis, on a component just inside the admission limit.  Every case here is a map plus points THERE, with the
winner of each point declared by hand where it can be (`winner`, -2 = not declared: the model decides).

Every map but the two `off.*` ones ENABLES the index: the component under test is accompanied by FILLERS, a lattice of 384 small
isotropic components a few metres away, so the mean list length stays under K / 24 and the global list under K / 4.  The cell size is
fixed with the option assoc_cell (CELL = 0.05 m), so the cases do not depend on the automatic choice.

  gate.tip.<cond>   an oblique needle (w0 ~ w1 << w2; axes ROT, none within 20 degrees of a grid axis) of condition 1e4 .. 9.9e7 whose
                    3-sigma long semi-axis is 1.2 m = 24 cells: 2 048 points along the long axis from 0.98 to 1.08 of the gate's
                    semi-axis at each tip, and at each tip a second, isotropic component whose chi2 = 9 sphere passes through the tip,
                    centred so that inside the tip chi2(needle) < chi2(second) <= 9
  gate.wide.8e+05   a needle of condition 8e5 at ROT_W: the one kind of component the index registers at a gate of ITS OWN.  Its error
                    bound (9.8e-4) is above the slack of 2.998e-6 and below the limit of 1e-3, and its computed chi2 at the + tip is
                    6.7e-6 below the exact one: the coarse scan of gate.tip plus 512 points per tip with chi2 from 9 (1 - 2e-6) to
                    9 (1 + 1.2e-5), of which dozens are resolved while they lie outside the ellipsoid at 9 (1 + 4e-6)
  gate.plane        the same for a plane-like component (w0 = 1e-6, w1 ~ w2), along each of its three principal axes
  gate.ellipsoid    ... and for a general ellipsoid
  gate.aabb         the six tangent points of the gate ellipsoid to its axis-aligned box, mu +- sqrt(T / cov_aa) cov[:, a], at the
                    relative distances 1 - 1e-7, 1 - 1e-9, 1 and 1 + 2e-6 from the mean: an oblique plane, an oblique ellipsoid and an
                    axis-aligned one.  The only points where condition (1) of the registration is tight
  edge.wide / .plain  a cell boundary put INSIDE a margin, where the registration's outer bound is tight.  Along x the box of the
                    component ends 1.5e-7 m (0.7e-7 m) short of a cell boundary if it is registered at 9 (1 + 4e-6) instead of its own
                    gate (at 9 instead of 9 (1 + 4e-6)); the point where the gate ellipsoid touches that side of its box, 2.6e-6
                    (2.5e-7) of the semi-axis farther out, lies just across the boundary and is resolved; a second component whose
                    computed chi2 there is larger and inside the gate shares the cell.  Two tiny fillers fix the grid's corners, so
                    the boundary does not move with the component.  edge.wide is gate.wide's needle (also through gl_track_frames:
                    its computed chi2 at the point is below 9), edge.plain the oblique ellipsoid
  admit.*           one component on each side of every admission decision, with the `always` count index_info() must report
  cell.list3/4      three / four concentric components over the same cells, with distinct chi2 and with an exact tie (duplicates: the
                    lowest index wins; at the common mean every chi2 is 0): the inline triple against the CSR list
  off.*             K = 5, and a map with more than a quarter of its components inadmissible: the index is NOT enabled
"""
import math

import numpy as np

from tests import assoc_model as am

f64 = np.float64
T = am.T_GATE
CELL = 0.05
C0 = np.array([0.0, 0.0, 8.0])  # where the component under test sits: in front of the camera of tests/optim_cases.py


def _rot(az, ay, ax):
    cz, sz, cy, sy, cx, sx = math.cos(az), math.sin(az), math.cos(ay), math.sin(ay), math.cos(ax), math.sin(ax)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    Ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return Rz @ Ry @ Rx


# (fixed; the error of the computed chi2 of a needle depends on how its covariance rounds: these angles are ones at which it shows)
ROT = _rot(math.radians(25.0), math.radians(35.0), math.radians(35.0))  # columns: the principal axes, thinnest first
assert np.abs(ROT).max() < math.cos(math.radians(20.0))  # no axis within 20 degrees of a grid axis


def comp(mu, lam, R=None):
    """(mean, cov) with the eigenvalues lam (ascending) on the columns of R; symmetric by construction"""
    R = np.eye(3) if R is None else R
    c = (R * np.asarray(lam, f64)) @ R.T
    return np.asarray(mu, f64), 0.5 * (c + c.T)


def iso(mu, s):
    return np.asarray(mu, f64), np.eye(3) * (s * s)


def fillers(x0=5.0):
    """384 isotropic components of 2 cm on a 0.5 m lattice, metres away from C0"""
    return [iso((x0 + 0.5 * i, -1.5 + 0.5 * j, 6.5 + 0.5 * k), 0.02) for i in range(8) for j in range(8) for k in range(6)]


class Case:
    def __init__(self, name, comps, pts, winner=None, options=None, enabled=True, always=None, under=(), track=False, by_box=0):
        self.name = name
        self.mean = np.ascontiguousarray(np.stack([c[0] for c in comps]), f64)
        self.cov = np.ascontiguousarray(np.stack([c[1] for c in comps]), f64)
        self.pts = np.ascontiguousarray(pts, f64).reshape(-1, 3)
        self.winner = -2 * np.ones(len(self.pts), np.int32) if winner is None else np.asarray(winner, np.int32)
        assert len(self.winner) == len(self.pts)
        self.options = dict(assoc_cell=CELL, **(options or {}))  # options the map is BUILT under
        self.enabled, self.always = enabled, always  # what index_info() must report
        self.by_box = by_box       # how many of `always` are there for their box (assoc_globcells), which am.admitted() does not model
        self.under = tuple(under)  # the components under test (the margin test takes every admitted component anyway)
        self.track = track         # goes through gl_track_frames too
        self._model = None

    def __repr__(self):
        return self.name

    @property
    def K(self):
        return len(self.mean)

    def model(self):
        """dict(idx, d2): the argmin and its chi2 by the bit-exact model, the lowest index on a tie; computed once"""
        if self._model is None:
            self._model = model_assoc(self.mean, self.cov, self.pts)
        return self._model


def model_assoc(mean, cov, pts):
    """The N x K sweep by tests/assoc_model.py.  numpy screens (on the model's own records, so only the summation order differs:
    its error is bounded per pair by the size of the terms), the model evaluates whatever could be the minimum."""
    recs = [am.record(m, c) for m, c in zip(mean, cov)]
    R = np.array(recs)
    A = R[:, 3:].reshape(-1, 3, 3)
    d = pts[:, None, :] - R[None, :, :3]
    with np.errstate(all="ignore"):
        q = np.einsum("nki,kij,nkj->nk", d, A, d)
        tol = 1e-13 * (d * d).sum(-1) * np.abs(A).max((1, 2))[None, :]
        hi = np.where(np.isfinite(q), q + tol, np.inf).min(1)
        cand = np.isfinite(q) & (q - tol <= hi[:, None])
    idx, d2 = np.zeros(len(pts), np.int32), np.zeros(len(pts))
    memo = {}
    for n in range(len(pts)):
        best, bi = math.inf, -1
        for k in np.nonzero(cand[n])[0]:
            key = (int(k), pts[n].tobytes())
            if key not in memo:
                memo[key] = am.chi2_device(recs[k], pts[n])
            v = memo[key]
            if v < best:  # ascending k: the first index of the minimum
                best, bi = v, int(k)
        idx[n], d2[n] = bi, best
    return dict(idx=idx, d2=d2)


CASES = {}


def add(case):
    assert case.name not in CASES
    CASES[case.name] = case
    return case


# ---- gate.tip ------------------------------------------------------------------------------------------------------------------------
W2 = 0.16                      # 3 sigma = 1.2 m = 24 cells
SEMI = math.sqrt(T * W2)
TIP_CONDS = (1e4, 1e6, 1e7, 3e7, 9.9e7)
NSCAN = 2048


def needle(cond, mu=C0):
    return comp(mu, (W2 / cond, 1.3 * W2 / cond, W2), ROT)


def scan(mu, axis, semi, n, lo=0.98, hi=1.08):
    """n points from lo to hi of the semi-axis at each tip: (2 n, 3), the + tip first"""
    f = np.linspace(lo, hi, n)
    return np.concatenate([mu + (f * semi)[:, None] * axis[None, :], mu - (f * semi)[:, None] * axis[None, :]])


def seconds(mu, axis, side, semi, s=0.1):
    """the isotropic component at each tip whose 3-sigma sphere passes through the tip, centred almost at right angles to the axis
    and slightly inwards (cos = -0.1): t inside the tip chi2(second) = 9 - 6 t + 100 t^2 against the needle's 9 - 15 t"""
    out = []
    for sgn in (1.0, -1.0):
        tip = mu + sgn * semi * axis
        out.append(iso(tip + 3.0 * s * (-0.1 * sgn * axis + math.sqrt(0.99) * side), s))
    return out


for _c in TIP_CONDS:
    _nd = needle(_c)
    add(Case("gate.tip.%.3g" % _c, [_nd] + seconds(C0, ROT[:, 2], ROT[:, 1], SEMI) + fillers(), scan(C0, ROT[:, 2], SEMI, NSCAN),
             always=0 if _c <= 1e4 else 1, under=(0,), track=True))

# ---- gate.wide: the needle registered at its own, wider gate ------------------------------------------------------------------------------
# (fixed like ROT: of the oblique rotations on a 5 degree lattice of the three angles the one whose needle of condition 8e5 has the most
# negative error at the + tip, -6.7e-6: more than twice the slack)
ROT_W = _rot(math.radians(35.0), math.radians(25.0), math.radians(55.0))
assert np.abs(ROT_W).max() < math.cos(math.radians(20.0))
WIDE_COND = 8e5
_f = np.concatenate([np.linspace(0.98, 1.08, 1536), np.linspace(1.0 - 1e-6, 1.0 + 6e-6, 512)])
_wide_pts = np.concatenate([C0 + sgn * (_f * SEMI)[:, None] * ROT_W[:, 2][None, :] for sgn in (1.0, -1.0)])
add(Case("gate.wide.%.3g" % WIDE_COND, [comp(C0, (W2 / WIDE_COND, 1.3 * W2 / WIDE_COND, W2), ROT_W)] + seconds(C0, ROT_W[:, 2], ROT_W[:, 1], SEMI) + fillers(),
         _wide_pts, always=0, under=(0,), track=True))

# ---- gate.plane / gate.ellipsoid -------------------------------------------------------------------------------------------------------
PLANE_LAM = (1e-6, 0.12, W2)
ELL_LAM = (1e-4, 4e-3, W2)
for _n, _lam in (("gate.plane", PLANE_LAM), ("gate.ellipsoid", ELL_LAM)):
    _pts = np.concatenate([scan(C0, ROT[:, a], math.sqrt(T * _lam[a]), 172) for a in range(3)])
    add(Case(_n, [comp(C0, _lam, ROT)] + seconds(C0, ROT[:, 2], ROT[:, 1], SEMI) + fillers(), _pts, always=0, under=(0,)))

# ---- gate.aabb -----------------------------------------------------------------------------------------------------------------------
AABB_F = (1.0 - 1e-7, 1.0 - 1e-9, 1.0, 1.0 + 2e-6)


def tangent_points(mu, cov):
    """mu +- f sqrt(T / cov_aa) cov[:, a]: where the gate ellipsoid touches its axis-aligned box, at the relative distances AABB_F"""
    return np.array([mu + sgn * f * math.sqrt(T / cov[a, a]) * cov[:, a] for a in range(3) for sgn in (1.0, -1.0) for f in AABB_F])


_ab = [comp(C0, PLANE_LAM, ROT), comp(C0 + (0.0, 2.75, 0.0), ELL_LAM, ROT), comp(C0 + (0.0, -2.75, 0.0), (4e-4, 1e-2, W2))]
add(Case("gate.aabb", _ab + fillers(), np.concatenate([tangent_points(*c) for c in _ab]), winner=np.repeat([0, 1, 2], 24), always=0,
         under=(0, 1, 2), track=True))

# ---- edge.*: a cell boundary inside a margin ---------------------------------------------------------------------------------------------
def edge_case(name, lam, R, gate_short, delta, f, second_chi2, track):
    """The component (lam, R) near C0, moved along x until the box it would have at the registration gate `gate_short` (over T) ends
    `delta` short of a cell boundary; point 0 is where the gate ellipsoid touches the +x side of its box, at f of the distance; the second
    component (0.1 m, isotropic, 0.3 m away along y) has chi2 = second_chi2 there.  The corners of the grid are two fillers of 1 mm."""
    rest = [iso((-1.5, -2.0, 6.0), 0.001), iso((6.0, 2.5, 10.0), 0.001)] + fillers(x0=2.0)
    mu, cov = comp(C0, lam, R)
    lo = am.grid_lo([mu] + [c[0] for c in rest], [cov] + [c[1] for c in rest])
    short = am.box_ext(cov, 0, gate_short)
    n = math.floor((mu[0] + short - lo[0]) / CELL) + 1
    mu = mu + ((lo[0] + n * CELL - delta) - (mu[0] + short), 0.0, 0.0)
    tangent = math.sqrt(T / cov[0, 0]) * cov[:, 0]
    pts = np.array([mu + f * tangent, mu + (1.0 - 1e-6) * tangent, mu + (1.0 + 8e-6) * tangent])
    second = iso(pts[0] + (0.0, 0.3 * math.sqrt(second_chi2 / T), 0.0), 0.1)
    comps = [(mu, cov), second] + rest
    # the construction holds: the corners are the fillers', point 0 is in cell n, the short box ends in cell n - 1, the box at the gate
    # the source registers this component at reaches cell n
    assert am.grid_lo([c[0] for c in comps], [c[1] for c in comps]) == lo
    assert math.floor((pts[0, 0] - lo[0]) / CELL) == n and math.floor((pts[1, 0] - lo[0]) / CELL) == n - 1
    assert am.box_last_cell(mu[0], short, lo[0], CELL) == n - 1
    assert am.box_last_cell(mu[0], am.box_ext(cov, 0, am.registered_gate(cov)), lo[0], CELL) >= n
    return add(Case(name, comps, pts, winner=[0, -2, -2], always=0, under=(0,), track=track))


_k = am.source_constants()
edge_case("edge.wide", (W2 / WIDE_COND, 1.3 * W2 / WIDE_COND, W2), ROT_W, 1.0 + _k["reg"], 1.5e-7, 1.0 + 2.6e-6, T * (1.0 - 2e-7), True)
edge_case("edge.plain", ELL_LAM, ROT, 1.0, 0.7e-7, 1.0 + 2.5e-7, T * (1.0 + 8e-7), False)


# ---- admit.* -------------------------------------------------------------------------------------------------------------------------
def around(mu, lam, R=None):
    """the mean, and 0.5 / 0.99 / 1.01 of the gate's semi-axis at both tips of each principal axis"""
    R = np.eye(3) if R is None else R
    return np.array([mu] + [mu + sgn * f * math.sqrt(T * lam[a]) * R[:, a] for a in range(3) for sgn in (1.0, -1.0) for f in (0.5, 0.99, 1.01)])


def admit(name, c, pts, always, winner=None, extra=(), **kw):
    return add(Case("admit." + name, [c] + list(extra) + fillers(), pts, always=always, winner=winner, under=(0,), **kw))


def _plane(cond):
    return (W2 / cond, 0.75 * W2, W2)


def _needle(cond):
    return (W2 / cond, 1.3 * W2 / cond, W2)


def _cond_at_err(err):
    """the condition number at which a needle of _needle() has the bound err: U (pair cond^2 / 1.3 + one cond) = err"""
    c = am.source_constants()
    a, b = c["err_pair"] / 1.3, c["err_one"]
    return (-b + math.sqrt(b * b + 4.0 * a * err / am.U)) / (2.0 * a)


# the condition limit 1e8, as plane (the bound on the error stays small: only the limit decides) and as needle (far above the
# error limit on either side: a needle leaves the grid long before)
admit("plane_below_cond", comp(C0, _plane(9.9e7), ROT), around(C0, _plane(9.9e7), ROT), always=0)
admit("plane_above_cond", comp(C0, _plane(1.01e8), ROT), around(C0, _plane(1.01e8), ROT), always=1)
admit("needle_below_cond", comp(C0, _needle(9.9e7), ROT), around(C0, _needle(9.9e7), ROT), always=1)
admit("needle_above_cond", comp(C0, _needle(1.01e8), ROT), around(C0, _needle(1.01e8), ROT), always=1)
# the limit on the error bound (kErrMax): the needle on either side of it, at 0.99 and 1.01 of the limit
ERR_CONDS = (_cond_at_err(0.99 * am.source_constants()["err_max"]), _cond_at_err(1.01 * am.source_constants()["err_max"]))
admit("needle_below_err", comp(C0, _needle(ERR_CONDS[0]), ROT), around(C0, _needle(ERR_CONDS[0]), ROT), always=0)
admit("needle_above_err", comp(C0, _needle(ERR_CONDS[1]), ROT), around(C0, _needle(ERR_CONDS[1]), ROT), always=1)
# the slack itself: the needle whose bound is 0.99 / 1.01 of it is registered at 9 (1 + 4e-6) / at a gate of its own.  Both are in
# the grid; what differs is the registered ellipsoid, which the model reads off the source (am.registered_gate)
SLACK_CONDS = (_cond_at_err(0.99 * am.source_constants()["slack"]), _cond_at_err(1.01 * am.source_constants()["slack"]))
admit("needle_below_slack", comp(C0, _needle(SLACK_CONDS[0]), ROT), around(C0, _needle(SLACK_CONDS[0]), ROT), always=0)
admit("needle_above_slack", comp(C0, _needle(SLACK_CONDS[1]), ROT), around(C0, _needle(SLACK_CONDS[1]), ROT), always=0)
# asym = |c01 - c10| + ... against 1e-12 w2: one off-diagonal entry of an axis-aligned ellipsoid
BLOB_LAM = (0.05, 0.1, W2)  # on z, y, x
for _n, _f, _alw in (("asym_below", 0.9e-12, 0), ("asym_above", 1.1e-12, 1)):
    _m, _cv = comp(C0, BLOB_LAM, np.eye(3)[:, ::-1])
    _cv[0, 1] = _f * W2
    admit(_n, (_m, _cv), around(C0, BLOB_LAM, np.eye(3)[:, ::-1]), always=_alw, winner=np.zeros(19, np.int32))
# one non-finite entry: on neither list, its chi2 is NaN for every point, a filler wins
_m, _cv = comp(C0, BLOB_LAM, np.eye(3)[:, ::-1])
_cv[0, 0] = np.inf
admit("nonfinite", (_m, _cv), around(C0, BLOB_LAM, np.eye(3)[:, ::-1]), always=0)
# w0 <= 0: singular (the inverse is not finite: never the minimum) and indefinite (chi2 is NEGATIVE along z: the minimum there)
admit("singular", comp(C0, (0.0, 0.1, W2), np.eye(3)[:, ::-1]), around(C0, (1e-4, 0.1, W2), np.eye(3)[:, ::-1]), always=1)
admit("indefinite", comp(C0, (-0.01, 0.1, W2), np.eye(3)[:, ::-1]), np.array([C0 + (0, 0, 0.25), C0 + (0, 0, -0.5), C0 + (0.5, 0, 0), C0 + (0.1, 0.1, 0.3)]),
      always=1, winner=np.zeros(4, np.int32))
# a box above assoc_globcells (set low: 1e6 cells): component 1 (sigma 1 m, a box of 121^3 cells) is evaluated for every point, component 0
# (sigma 0.5 m) is registered.  The point 1 m from component 0 and 2 m from component 1 has chi2 = 4.0 exactly for both: index 0 wins,
# although the global list is evaluated first
admit("box", iso(C0, 0.5), np.array([C0 + (1.0, 0, 0), C0 + (0.5, 0, 0), C0 + (1.25, 0, 0), C0 + (3.0, 0.5, 0)]), always=1,
      winner=np.array([0, 0, 1, 1], np.int32), extra=[iso(C0 + (3.0, 0, 0), 1.0)], options=dict(assoc_globcells=1e6), by_box=1)
add(Case("admit.box_default", [iso(C0, 0.5), iso(C0 + (3.0, 0, 0), 1.0)] + fillers(), CASES["admit.box"].pts, always=0,
         winner=np.array([0, 0, 1, 1], np.int32), under=(0, 1)))

# ---- cell.list3 / cell.list4 -----------------------------------------------------------------------------------------------------------
_off = np.array([(0, 0, 0), (0.01, 0.02, 0.03), (-0.11, 0.07, 0.02), (0.2, -0.1, 0.15), (0.0, 0.29, 0.0), (0.0, 0.0, -0.59)])
C1 = C0 + (0.0, 2.75, 0.0)
# distinct: the widest component has the smallest chi2 away from the mean; AT the mean every chi2 is 0.0 and the lowest index wins
add(Case("cell.list3", [iso(C0, 0.05), iso(C0, 0.1), iso(C0, 0.2)] + [iso(C1, 0.1), iso(C1, 0.2), iso(C1, 0.2)] + fillers(),
         np.concatenate([C0 + _off, C1 + _off]), winner=[0, 2, 2, 2, 2, 2] + [3, 4, 4, 4, 4, 4], always=0, under=range(6)))
add(Case("cell.list4", [iso(C0, 0.05), iso(C0, 0.1), iso(C0, 0.2), iso(C0, 0.15)] + [iso(C1, 0.05), iso(C1, 0.2), iso(C1, 0.1), iso(C1, 0.2)] + fillers(),
         np.concatenate([C0 + _off, C1 + _off]), winner=[0, 2, 2, 2, 2, 2] + [4, 5, 5, 5, 5, 5], always=0, under=range(8)))

# ---- off.*: maps on which build_cell_index does NOT enable the index ---------------------------------------------------------------------
_five = [iso(C0 + (0.7 * i, 0, 0), 0.1) for i in range(5)]
add(Case("off.k5", _five, np.array([c[0] + (0.05, 0.02, 0.0) for c in _five]), winner=np.arange(5), enabled=False))  # a list of 1 > 5 / 24
_q = fillers()[:8]
for _i in (1, 4, 6):  # 3 of 8 on the global list: more than K / 4
    _q[_i] = (_q[_i][0], np.diag([4e-4, 4e-4, 0.0]))
add(Case("off.quarter", _q, np.array([c[0] + (0.01, 0.0, 0.0) for c in _q]), enabled=False))


def names(prefix=""):
    return [n for n in CASES if n.startswith(prefix)]


# ---- the points of a gate.tip scan the index could lose ------------------------------------------------------------------------------
T_RESOLVE = T * (1.0 + am.source_constants()["resolve"])  # the expressions of gl_grid.hip
T_REG = T * (1.0 + am.source_constants()["reg"])
_tip = {}


def tip_sets(case):
    """For a gate.tip case, by the model: dict(dev, sec, lost, between).  dev / sec: the computed chi2 of every scan point against the
    needle and against the second component of its tip.  lost: computed chi2(needle) <= 9 (1 + 1e-6) while the exact chi2 is above
    9 (1 + 4e-6) - resolved by the index, outside the ellipsoid at the plain registration gate; lost_own: the same against the gate
    this component is registered at (am.registered_gate).  between: chi2(needle) < chi2(second) <= 9 (1 + 1e-6)
    as computed - if the needle's list misses the point's cell, the index reports the second component."""
    if case.name not in _tip:
        rec = [am.record(case.mean[k], case.cov[k]) for k in range(3)]
        n2 = len(case.pts) // 2
        dev = np.array([am.chi2_device(rec[0], p) for p in case.pts])
        sec = np.array([am.chi2_device(rec[1 if n < n2 else 2], p) for n, p in enumerate(case.pts)])
        ex = [am.chi2_exact(case.cov[0], case.mean[0], p) if d <= T_RESOLVE else None for d, p in zip(dev, case.pts)]
        lost = np.array([e is not None and e > am.Fr(T_REG) for e in ex])
        t_own = am.Fr(T) * am.Fr(am.registered_gate(case.cov[0]))  # where the source registers THIS component
        _tip[case.name] = dict(dev=dev, sec=sec, lost=lost, lost_own=np.array([e is not None and e > t_own for e in ex]),
                               between=(dev < sec) & (sec <= T_RESOLVE))
    return _tip[case.name]


def track_points(case, per=4):
    """the points of a case that go through gl_track_frames: of a tip scan the first `per` lost and between points of each tip and the
    points on either side of the computed gate; every point of gate.aabb's component at C0 and the f = 1 points of the other two"""
    if case.name == "gate.aabb":
        return list(range(24)) + [n for n in range(24, 72) if n % 4 == 2]
    if case.name.startswith("edge."):
        return [0, 1, 2]
    s, n2 = tip_sets(case), len(case.pts) // 2
    out = []
    for lo in (0, n2):
        for m in (s["lost"], s["between"]):
            out += list(lo + np.nonzero(m[lo:lo + n2])[0][:per])
        cross = lo + int(np.argmax(s["dev"][lo:lo + n2] > T))
        out += [max(lo, cross - 1), cross]
    return sorted(set(int(n) for n in out))


# ---- gl_track_frames -------------------------------------------------------------------------------------------------------------------
TRACK_SLOT = 5


def track_scene(case, n):
    """The exactly projecting scene of tests/optim_cases.py (twelve points, each on an anchor blob) with point TRACK_SLOT moved onto point n
    of the case; the map is the case's with the eleven other anchors appended (the indices of the case's components stay)."""
    from tests import optim_cases as oc
    X = oc.grid()
    X[TRACK_SLOT] = case.pts[n]
    d = oc.track_data(oc.anchors(skip=(TRACK_SLOT,)), X=X)
    d["mean"] = np.concatenate([case.mean, d["mean"]])
    d["cov"] = np.concatenate([case.cov, np.asarray(d["cov"], f64).reshape(-1, 3, 3)])
    return d
