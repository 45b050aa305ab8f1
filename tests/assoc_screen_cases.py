"""Hand-built maps and points for GL_ASSOC_SCREENED (gmmloc_amd/csrc/gl_assoc32.hip): the families of pairs on which its fp32 bound
is held to exact arithmetic, and the cases whose counters GL_COUNTER_ASSOC_SCREEN_VERIFIED / _FALLBACK are declared, for
tests/test_assoc_screen_cases.py (CPU: the model of tests/assoc_screen_model.py) and tests/test_gpu_assoc_screen_cases.py (the
device must reproduce every declared integer).  Test infrastructure.

A case is a map, a handful of declared points, the length N of the call (the declared points repeated in turn, so every lane and
both halves of a packed pair see each of them and the counters are sums of the per-point figures) and, per declared point,
(idx, verified, fallback): DECLARED below, by hand where the scene makes it obvious (HAND has those idx), by the model otherwise and
then pinned.  `shape` is the launch shape the case was built to reach; both tests assert it, so no case passes vacuously.

  ladder.K<k>.*   two equal oblique components and a point walked along x across the place where lo_1 meets U = hi_0: two ADJACENT
                  doubles of x, lo_1 == U exactly on one (admitted: the test is !(l > U); verified 2) and one fp32 ulp above on the
                  other (verified 1).  K = 2 .. 8, N = 1, and N = 2 with the point in either half of the pair.  ladder.near is
                  the same 5e-4 m from a mean, where e is of the size of s and the roundings of n and E decide as well.  DECIDES
                  lists, per ladder, the intermediates whose change by one ulp changes the count (found by search in the model)
  tail.*          K = 9 and 15: a last chunk of 1 and of 7 components, the winner in it, duplicates at k = 7 and 8
  split.K*        K = 65, 72, 128, 129 (2, 2, 2, 3 splits): the winner in the last split's last chunk, duplicates on either side
                  of a split boundary, U from a wide component in split 0 while the narrow winner sits in the last split
  kout.32 / .40   32 identical components (4 chunks, all handed on: verified 32) and 40 (5 chunks: one has no room, fallback)
  compact.cap8    K = 2 304, N = 8 191 (k_assoc_screen<1>, 9 chunks per split, list of 8): regions a few metres apart, region r using
  compact.cap4    component 8 j + r of chunk j; K = 80, N = 16 384 (k_assoc_screen<2>, 5 chunks per split, list of 4).  A descending
                  staircase longer than the list (compaction drops every entry), one exactly as long as the list, a plateau of tied
                  chunks longer than the list (fallback, lowest index), one exactly as long, a staircase that ends in three tied
                  chunks (compaction keeps two entries and MOVES them), and - cap4 only - a plateau whose second chunk holds a
                  ladder component with lo == U exactly: kept by the compaction, so the last chunk has no room (fallback); one ulp
                  above it was never noted (no fallback)
  lanes.K*        K = 256, 257, 1 024, 1 025, 2 049 (L = 1, 2, 4, 8, 16 lanes per point in the verify kernel): duplicates in splits
                  of different lanes with the lowest k in the lower and in the higher lane, in three lanes, and a point whose only
                  candidate lies in the last split of the last lane
  gate.point      a point on either side of big <= 1e37 (adjacent doubles); gate.map.*: a map on either side of
                  cmax rmax^2 < 1e30 (adjacent doubles of a mean)
"""
import math

import numpy as np

from tests import assoc_cases as ac
from tests import assoc_screen_model as sm

f64 = np.float64
ISO = 0.01  # variance of the plain components: sigma = 0.1 m


# ---- deterministic pieces (no BLAS, no libm: the ladders depend on every bit of the map) ---------------------------------------------------
R3 = [[2.0 / 3.0, -1.0 / 3.0, 2.0 / 3.0], [2.0 / 3.0, 2.0 / 3.0, -1.0 / 3.0], [-1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0]]  # a rotation, oblique to every axis


def cov_of(lam, R=R3):
    """R diag(lam) R^T with the sums in a fixed order, symmetric by construction"""
    c = [[(R[i][0] * lam[0] * R[j][0] + R[i][1] * lam[1] * R[j][1]) + R[i][2] * lam[2] * R[j][2] for j in range(3)] for i in range(3)]
    return np.array([[c[min(i, j)][max(i, j)] for j in range(3)] for i in range(3)], f64)


def iso(s2=ISO):
    return np.eye(3) * s2


def filler(k):
    """the components no declared point comes near: sigma 0.1 on a 1 m lattice 170 m away"""
    return (100.0 + k % 16, 100.0 + (k // 16) % 16, 100.0 + k // 256), iso()


def build_map(K, placed):
    comps = [placed[k] if k in placed else filler(k) for k in range(K)]
    return (np.ascontiguousarray([c[0] for c in comps], f64), np.ascontiguousarray([c[1] for c in comps], f64))


class Case:
    def __init__(self, name, mean, cov, pts, N, shape, brute=False, reach=None, has_records=True):
        self.name, self.mean, self.cov = name, np.ascontiguousarray(mean, f64), np.ascontiguousarray(cov, f64).reshape(-1, 3, 3)
        self.pts, self.N, self.shape, self.brute = np.ascontiguousarray(pts, f64).reshape(-1, 3), N, shape, brute
        self.reach = reach or {}  # declared point -> dict(split=, compactions=, peak=): the path through note() it was built to take
        self.has_records = has_records
        self._map = self._ref = None
        self._model = {}

    def __repr__(self):
        return self.name

    @property
    def K(self):
        return len(self.mean)

    def full_points(self):
        """the N points of the call: the declared points in turn"""
        return np.ascontiguousarray(self.pts[np.arange(self.N) % len(self.pts)])

    def multiplicity(self):
        return np.bincount(np.arange(self.N) % len(self.pts), minlength=len(self.pts))

    def map(self):
        if self._map is None:
            self._map = sm.ScreenMap(self.mean, self.cov)
        return self._map

    def reference(self):
        """idx, d2 of the exhaustive sweep by the bit-exact model of tests/assoc_model.py (the lowest index on a tie)"""
        if self._ref is None:
            with np.errstate(all="ignore"):
                self._ref = ac.model_assoc(self.mean, self.cov.reshape(-1, 9), self.pts)
        return self._ref

    def model(self, **mutation):
        """the screen model's Result per declared point"""
        key = tuple(sorted(mutation.items()))
        if key not in self._model:
            ref = self.reference()
            self._model[key] = [sm.associate_point(self.map(), p, self.N, reference=(int(ref["idx"][i]), float(ref["d2"][i])), **mutation)
                                for i, p in enumerate(self.pts)]
        return self._model[key]

    def counters(self, declared=None):
        """(verified, fallback) of the whole call from the per-point declarations"""
        d = DECLARED[self.name] if declared is None else declared
        mult = self.multiplicity()
        return int(sum(m * v for m, (_, v, _) in zip(mult, d))), int(sum(m * f for m, (_, _, f) in zip(mult, d)))


CASES = {}


def add(c):
    assert c.name not in CASES, c.name
    CASES[c.name] = c
    return c


def names(prefix=""):
    return sorted(n for n in CASES if n.startswith(prefix))


def shape(ppt, nsplit, kchunk, chunks, L):
    return dict(ppt=ppt, nsplit=nsplit, kchunk=kchunk, chunks=chunks, L=L, cap=8 // (ppt // 2))


# ---- 1. ladders ------------------------------------------------------------------------------------------------------------------------------
LADDER_SEP = (1.0, 0.25, -0.125)
LADDER_LAM = (0.01, 0.02, 0.05)


def ladder_map(K, sc):
    """components 0 and 1 with the same oblique covariance (LADDER_LAM scaled by sc), LADDER_SEP apart; the others 4 m and more to the side"""
    cv = cov_of([l * sc for l in LADDER_LAM])
    mean = [(0.0, 0.0, 0.0), LADDER_SEP] + [(0.5, 4.0 + j, 0.0) for j in range(K - 2)]
    return np.array(mean, f64), np.array([cv] * K)


def near_map():
    mean = [(0.0, 0.0, 0.0), (5e-4, 0.0, 0.0), (-0.5, 0.0, 0.0), (0.5, 0.0, 0.0)]
    return np.array(mean, f64), np.array([iso()] * 4)


LADDER_PARTNER = (0.03125, -0.015625, 0.0078125)  # the other point of an N = 2 call: near component 0, verified 1
GROUPS = dict(D=("d0", "d1", "d2"), t=("t0a", "t0b", "t0", "t1a", "t1", "t2"), s=("s0", "s1", "s"), nE=("n0", "n1", "n", "E"), hilo=("hi", "lo"))


def _ladder_cases():
    one_chunk = lambda K: shape(2, 1, (K + 7) // 8 * 8, 1, 1)
    for K, (sc, x_eq, x_up) in sorted(LADDERS.items()):
        assert abs(x_eq - x_up) == math.ulp(min(x_eq, x_up))
        mean, cov = ladder_map(K, sc)
        y, z = 0.5 * LADDER_SEP[1], 0.5 * LADDER_SEP[2]
        eq, up = (x_eq, y, z), (x_up, y, z)
        add(Case("ladder.K%d.n1.eq" % K, mean, cov, [eq], 1, one_chunk(K), brute=True))
        add(Case("ladder.K%d.n1.up" % K, mean, cov, [up], 1, one_chunk(K), brute=True))
        for side, p in (("eq", eq), ("up", up)):
            add(Case("ladder.K%d.n2.%s.x" % (K, side), mean, cov, [p, LADDER_PARTNER], 2, one_chunk(K), brute=True))
            add(Case("ladder.K%d.n2.%s.y" % (K, side), mean, cov, [LADDER_PARTNER, p], 2, one_chunk(K), brute=True))
    mean, cov = near_map()
    add(Case("ladder.near.eq", mean, cov, [NEAR[0], NEAR[1]], 2, one_chunk(4), brute=True))
    add(Case("ladder.near.up", mean, cov, [NEAR[1], NEAR[0]], 2, one_chunk(4), brute=True))


# ---- 2. - 6.: regions ---------------------------------------------------------------------------------------------------------------------------
OFF = (0.03125, -0.015625, 0.0078125)  # where a point sits relative to the mean it is meant for: chi2 = 0.13


def at(c, d=(0.0, 0.0, 0.0)):
    return (c[0] + d[0], c[1] + d[1], c[2] + d[2])


def centre(r):
    return (12.0 * r, 0.0, 0.0)


def _tail_cases():
    A, B = centre(0), centre(1)
    for K, last in ((9, 8), (15, 14)):
        mean, cov = build_map(K, {last: (A, iso()), 7: (B, iso())})
        add(Case("tail.K%d.winner" % K, mean, cov, [at(A, OFF), at(B, OFF)], 2, shape(2, 1, 16, 2, 1), brute=True))
        mean, cov = build_map(K, {last: (A, iso()), 7: (B, iso()), 8: (B, iso())} if K == 15 else {7: (B, iso()), 8: (B, iso())})
        add(Case("tail.K%d.dup" % K, mean, cov, [at(B, OFF), at(B)], 2, shape(2, 1, 16, 2, 1), brute=True))


def _split_cases():
    A, B, C = centre(0), centre(1), centre(2)
    for K, (nsplit, kchunk) in ((65, (2, 40)), (72, (2, 40)), (128, (2, 64)), (129, (3, 48))):
        pc = at(C, (0.17, 0.0, 0.0))  # chi2 2.89 to the wide component at C; the narrow one (sigma 1 mm) is 1 mm from it: chi2 1
        placed = {K - 1: (A, iso()), kchunk - 1: (B, iso()), kchunk: (B, iso()), 3: (C, iso()), K - 3: (at(pc, (0.0, 0.001, 0.0)), iso(1e-6))}
        mean, cov = build_map(K, placed)
        add(Case("split.K%d" % K, mean, cov, [at(A, OFF), at(B, OFF), pc], 3, shape(2, nsplit, kchunk, kchunk // 8, 1), brute=True))


def _kout_cases():
    A = centre(0)
    for K, chunks in ((32, 4), (40, 5)):
        mean, cov = build_map(K, {k: (A, iso()) for k in range(K)})
        add(Case("kout.%d" % K, mean, cov, [at(A, OFF)], 1, shape(2, 1, K, chunks, 1), brute=True))




def _staircase(placed, pts, r, first_chunk, steps, tied=0):
    """region r: a component in each of `steps` consecutive chunks at 0.1 (steps - j) m from the point (chi2 100 d^2: every later
    chunk rules the earlier ones out), then `tied` more chunks each holding a copy of the last step's component (0.1 m: chi2 1)"""
    c = centre(r)
    for j in range(steps + tied):
        placed[8 * (first_chunk + j) + r] = (at(c, (0.1 * (steps - min(j, steps - 1)), 0.0, 0.0)), iso())
    pts.append(c)


def compact_parts(per, cap, tie_sc=None):
    """the placed components, the declared points (without the two of the tie) and the path each takes through note()"""
    placed, pts = {}, []
    _staircase(placed, pts, 0, 0, per)                    # longer than the list by one: compaction, every entry dropped
    _staircase(placed, pts, 1, 0, cap)                    # exactly as long as the list
    _staircase(placed, pts, 2, 0, 1, tied=per - 1)        # a plateau longer than the list: no entry can go, fallback
    _staircase(placed, pts, 3, 0, 1, tied=cap - 1)        # a plateau exactly as long
    _staircase(placed, pts, 4, per, per - 2, tied=2)      # in split 1: the compaction keeps the two tied entries and moves them
    reach = {0: dict(split=0, compactions=1, peak=cap), 1: dict(split=0, compactions=0, peak=cap), 2: dict(split=0, compactions=1, peak=cap),
             3: dict(split=0, compactions=0, peak=cap), 4: dict(split=1, compactions=1, peak=cap)}
    if tie_sc is not None:  # region 5, split 0: copies of ladder component 0 in every chunk but the second, ladder component 1 there
        cv = cov_of([l * tie_sc for l in LADDER_LAM])
        for j in range(per):
            placed[8 * j + 5] = (at(TIE_C, LADDER_SEP), cv) if j == 1 else (TIE_C, cv)
        reach[5] = dict(split=0, compactions=1, peak=cap)
        reach[6] = dict(split=0, compactions=0, peak=cap)
    return placed, pts, reach


TIE_C = (57.55, 52.0, 50.0)  # the origin of the cap4 map: P is small there and moves in steps as fine as a ladder's


def tie_point(x):
    return (x, TIE_C[1] + 0.5 * LADDER_SEP[1], TIE_C[2] + 0.5 * LADDER_SEP[2])


def _compact_case(name, K, N, cap, sh, tie=None):
    placed, pts, reach = compact_parts(sh["chunks"], cap, tie[0] if tie else None)
    if tie:
        assert abs(tie[1] - tie[2]) == math.ulp(min(tie[1], tie[2]))
        pts += [tie_point(tie[1]), tie_point(tie[2])]
    mean, cov = build_map(K, placed)
    return add(Case(name, mean, cov, pts, N, sh, reach=reach))


def _compact_cases():
    _compact_case("compact.cap8", 2304, 8191, 8, shape(2, 32, 72, 9, 8))
    _compact_case("compact.cap4", 80, 16384, 4, shape(4, 2, 40, 5, 1), tie=COMPACT_TIE)


def _lane_cases():
    for K, (nsplit, kchunk, L) in ((256, (4, 64, 1)), (257, (5, 56, 2)), (1024, (16, 64, 4)), (1025, (17, 64, 8)), (2049, (33, 64, 16))):
        first = lambda s: s * kchunk  # the first component of split s
        last_lane_split = max(s for s in range(nsplit) if s % L == L - 1)
        placed = {}
        groups = [(1, L), (0, max(L - 1, 1)), (last_lane_split,), (max(L - 1, 0), L, L + 1)] if L > 1 else [(1, 2), (0, 3), (3,), (0, 1, 2)]
        for r, splits in enumerate(groups):  # region r: the same component at k = first(s) + r for each of its splits
            for s in splits:
                placed[first(s) + r] = (centre(r), iso())
        # the lowest k sits in the higher lane in groups 0 (split 1 against L) and 3 (L - 1 against L and L + 1), in the lower lane in group 1
        mean, cov = build_map(K, placed)
        add(Case("lanes.K%d" % K, mean, cov, [at(centre(r), OFF) for r in range(4)], 4, shape(2, nsplit, kchunk, kchunk // 8, L), brute=True))
        LANE_HAND["lanes.K%d" % K] = [min(first(s) + r for s in splits) for r, splits in enumerate(groups)]


LANE_HAND = {}


def gate_point_map():
    return np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)], f64), np.array([iso()] * 2)


def gate_map(x):
    """two components of sigma 0.1 mm (cmax 1e8) x apart: rmax = x / 2"""
    return np.array([(0.0, 0.0, 0.0), (x, 0.0, 0.0)], f64), np.array([iso(1e-8)] * 2)


def _gate_cases():
    assert abs(GATE_POINT[0] - GATE_POINT[1]) == math.ulp(GATE_POINT[0])
    mean, cov = gate_point_map()
    add(Case("gate.point", mean, cov, [(GATE_POINT[0], 0.0, 0.0), (GATE_POINT[1], 0.0, 0.0), OFF], 3, shape(2, 1, 8, 1, 1)))
    assert abs(GATE_MAP[0] - GATE_MAP[1]) == math.ulp(GATE_MAP[0])
    pts = [OFF, (2e-4, 1e-4, 0.0), at((GATE_MAP[0], 0.0, 0.0), (1e-4, 0.0, 2e-4))]
    for tag, x, has in (("below", GATE_MAP[0], True), ("above", GATE_MAP[1], False)):
        mean, cov = gate_map(x)
        add(Case("gate.map." + tag, mean, cov, pts, 3, shape(2, 1, 8, 1, 1), has_records=has))


# ---- the pinned figures ------------------------------------------------------------------------------------------------------------------------------
# Found by bisection in the model and pinned; tests/test_assoc_screen_cases.py asserts every property they were searched for.
#   LADDERS[K] = (sc, x with lo_1 == U, x with lo_1 one ulp above U): adjacent doubles (y, z: half of LADDER_SEP)
#   NEAR = (point with lo_1 == U, point one ulp above);  COMPACT_TIE = (sc, x with lo == U, x one ulp above) of region 5 of compact.cap4
#   GATE_POINT = (x with big <= 1e37, the next double);  GATE_MAP = (x of the second mean with cmax rmax^2 < 1e30, the next double)
#   DECIDES: ladder -> the groups of intermediates (GROUPS) whose change by one ulp changes `verified` / `fallback`
LADDERS = {2: (1.2568223476409912, 0.4999994188547419, 0.49999941885474186),
           3: (1.6889928579330444, 0.499998375773373, 0.49999837577337297),
           4: (1.5380481481552124, 0.4999980628489311, 0.49999806284893106),
           5: (0.637243390083313, 0.49999774992477347, 0.4999977499247734),
           6: (1.3117157220840454, 0.4999974519015496, 0.49999745190154954),
           7: (1.2616583108901978, 0.4999971240757759, 0.49999712407577585),
           8: (1.8070091009140015, 0.499996826052552, 0.49999682605255197)}
NEAR = ((9.946772115654312e-05, 2.829275525031083e-06, 3.924483801180455e-06), (9.946772115654311e-05, 2.829275525031083e-06, 3.924483801180455e-06))
COMPACT_TIE = (1.6738864183425903, 58.049981626868245, 58.04998162686824)
GATE_POINT = (59845585966774.78, 59845585966774.79)
GATE_MAP = (199999903999.86908, 199999903999.8691)
DECIDES = {K: ["D", "t", "s", "hilo"] for K in LADDERS}
DECIDES["near"] = ["D", "t", "s", "nE", "hilo"]
DECIDES["tie"] = ["D", "t", "s", "hilo"]
# per declared point (idx, verified, fallback): what the device's counters must add up to
DECLARED = {
    'compact.cap4': [(32, 1, 0), (25, 1, 0), (2, 0, 1), (3, 4, 0), (60, 3, 0), (5, 0, 1), (5, 4, 0)],
    'compact.cap8': [(64, 1, 0), (57, 1, 0), (2, 0, 1), (3, 0, 1), (124, 3, 0)],
    'gate.map.above': [(0, 0, 1), (0, 0, 1), (1, 0, 1)],
    'gate.map.below': [(0, 2, 0), (0, 2, 0), (1, 2, 0)],
    'gate.point': [(1, 2, 0), (1, 0, 1), (0, 1, 0)],
    'kout.32': [(0, 32, 0)],
    'kout.40': [(0, 0, 1)],
    'ladder.K2.n1.eq': [(0, 2, 0)],
    'ladder.K2.n1.up': [(0, 1, 0)],
    'ladder.K2.n2.eq.x': [(0, 2, 0), (0, 1, 0)],
    'ladder.K2.n2.eq.y': [(0, 1, 0), (0, 2, 0)],
    'ladder.K2.n2.up.x': [(0, 1, 0), (0, 1, 0)],
    'ladder.K2.n2.up.y': [(0, 1, 0), (0, 1, 0)],
    'ladder.K3.n1.eq': [(0, 2, 0)],
    'ladder.K3.n1.up': [(0, 1, 0)],
    'ladder.K3.n2.eq.x': [(0, 2, 0), (0, 1, 0)],
    'ladder.K3.n2.eq.y': [(0, 1, 0), (0, 2, 0)],
    'ladder.K3.n2.up.x': [(0, 1, 0), (0, 1, 0)],
    'ladder.K3.n2.up.y': [(0, 1, 0), (0, 1, 0)],
    'ladder.K4.n1.eq': [(0, 2, 0)],
    'ladder.K4.n1.up': [(0, 1, 0)],
    'ladder.K4.n2.eq.x': [(0, 2, 0), (0, 1, 0)],
    'ladder.K4.n2.eq.y': [(0, 1, 0), (0, 2, 0)],
    'ladder.K4.n2.up.x': [(0, 1, 0), (0, 1, 0)],
    'ladder.K4.n2.up.y': [(0, 1, 0), (0, 1, 0)],
    'ladder.K5.n1.eq': [(0, 2, 0)],
    'ladder.K5.n1.up': [(0, 1, 0)],
    'ladder.K5.n2.eq.x': [(0, 2, 0), (0, 1, 0)],
    'ladder.K5.n2.eq.y': [(0, 1, 0), (0, 2, 0)],
    'ladder.K5.n2.up.x': [(0, 1, 0), (0, 1, 0)],
    'ladder.K5.n2.up.y': [(0, 1, 0), (0, 1, 0)],
    'ladder.K6.n1.eq': [(0, 2, 0)],
    'ladder.K6.n1.up': [(0, 1, 0)],
    'ladder.K6.n2.eq.x': [(0, 2, 0), (0, 1, 0)],
    'ladder.K6.n2.eq.y': [(0, 1, 0), (0, 2, 0)],
    'ladder.K6.n2.up.x': [(0, 1, 0), (0, 1, 0)],
    'ladder.K6.n2.up.y': [(0, 1, 0), (0, 1, 0)],
    'ladder.K7.n1.eq': [(0, 2, 0)],
    'ladder.K7.n1.up': [(0, 1, 0)],
    'ladder.K7.n2.eq.x': [(0, 2, 0), (0, 1, 0)],
    'ladder.K7.n2.eq.y': [(0, 1, 0), (0, 2, 0)],
    'ladder.K7.n2.up.x': [(0, 1, 0), (0, 1, 0)],
    'ladder.K7.n2.up.y': [(0, 1, 0), (0, 1, 0)],
    'ladder.K8.n1.eq': [(0, 2, 0)],
    'ladder.K8.n1.up': [(0, 1, 0)],
    'ladder.K8.n2.eq.x': [(0, 2, 0), (0, 1, 0)],
    'ladder.K8.n2.eq.y': [(0, 1, 0), (0, 2, 0)],
    'ladder.K8.n2.up.x': [(0, 1, 0), (0, 1, 0)],
    'ladder.K8.n2.up.y': [(0, 1, 0), (0, 1, 0)],
    'ladder.near.eq': [(0, 2, 0), (0, 1, 0)],
    'ladder.near.up': [(0, 1, 0), (0, 2, 0)],
    'lanes.K1024': [(64, 2, 0), (1, 2, 0), (962, 1, 0), (195, 3, 0)],
    'lanes.K1025': [(64, 2, 0), (1, 2, 0), (962, 1, 0), (451, 3, 0)],
    'lanes.K2049': [(64, 2, 0), (1, 2, 0), (1986, 1, 0), (963, 3, 0)],
    'lanes.K256': [(64, 2, 0), (1, 2, 0), (194, 1, 0), (3, 3, 0)],
    'lanes.K257': [(56, 2, 0), (1, 2, 0), (170, 1, 0), (59, 3, 0)],
    'split.K128': [(127, 1, 0), (63, 2, 0), (125, 2, 0)],
    'split.K129': [(128, 1, 0), (47, 2, 0), (126, 2, 0)],
    'split.K65': [(64, 1, 0), (39, 2, 0), (62, 2, 0)],
    'split.K72': [(71, 1, 0), (39, 2, 0), (69, 2, 0)],
    'tail.K15.dup': [(7, 2, 0), (7, 2, 0)],
    'tail.K15.winner': [(14, 1, 0), (7, 1, 0)],
    'tail.K9.dup': [(7, 2, 0), (7, 2, 0)],
    'tail.K9.winner': [(8, 1, 0), (7, 1, 0)],
}

_ladder_cases()
_tail_cases()
_split_cases()
_kout_cases()
_compact_cases()
_lane_cases()
_gate_cases()

# idx declared by hand, where the scene makes it obvious (None: the model's)
HAND = {}
for _n in names("ladder."):
    HAND[_n] = [0] * len(CASES[_n].pts)  # every ladder point is on component 0's side of the middle
HAND.update({"tail.K9.winner": [8, 7], "tail.K15.winner": [14, 7], "tail.K9.dup": [7, 7], "tail.K15.dup": [7, 7],
             "split.K65": [64, 39, 62], "split.K72": [71, 39, 69], "split.K128": [127, 63, 125], "split.K129": [128, 47, 126],
             "kout.32": [0], "kout.40": [0]})
HAND.update(LANE_HAND)
HAND["compact.cap8"] = [64, 57, 2, 3, 8 * 15 + 4]
HAND["compact.cap4"] = [32, 25, 2, 3, 8 * 7 + 4, 5, 5]


# ---- the families of pairs for the bound ------------------------------------------------------------------------------------------------------------
def quat_rot(rng):
    """a Haar rotation from a normalised Gaussian quaternion, elementwise arithmetic only"""
    w, x, y, z = (float(v) for v in rng.standard_normal(4))
    n = math.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def _unit(rng):
    v = rng.standard_normal(3)
    return v / math.sqrt(float(v @ v))


FAMILY_SEED = dict(iso=11, aniso=12, offdiag=13, far=14, near=15, gate=16)
WELL_SCALED = ("iso", "offdiag")  # also held to chi2_exact


def family(name):
    """yields (mean (K, 3), cov (K, 3, 3), points (P, 3)): every point is paired with every component.  Pinned seeds."""
    rng = np.random.default_rng(FAMILY_SEED[name])
    if name == "iso":  # ||D|| from 1e-3 to 3 on maps of extent 0.01, 1, 6, 100: the u term and the beta term of G dominate in turn
        for ext in (0.01, 1.0, 6.0, 100.0):
            for _ in range(14):
                mean = rng.uniform(-0.5 * ext, 0.5 * ext, (6, 3))
                cov = np.array([iso(float(10.0 ** rng.uniform(-4, 0))) for _ in range(6)])
                pts = [mean[i % 6] + _unit(rng) * 10.0 ** rng.uniform(-3, math.log10(3.0)) for i in range(10)]
                yield mean, cov, np.array(pts)
    elif name == "aniso":  # needles, discs, ellipsoids of condition 1e4 .. 1e10 under Haar rotations
        for kind in ("needle", "disc", "full"):
            for cond in (1e4, 1e6, 1e8, 1e10):
                for _ in range(5):
                    big = float(10.0 ** rng.uniform(-2, 0))
                    lam = dict(needle=(big / cond, 1.3 * big / cond, big), disc=(big / cond, 0.7 * big, big),
                               full=(big / cond, big / math.sqrt(cond), big))[kind]
                    Rs = [quat_rot(rng) for _ in range(6)]
                    mean = rng.uniform(-3, 3, (6, 3))
                    cov = np.array([cov_of(lam, R) for R in Rs])
                    pts = []
                    for i in range(9):
                        R, m = np.array(Rs[i % 6]), mean[i % 6]
                        t = rng.uniform(0.1, 4.0)
                        if i % 3 == 0:    # along the stiffest axis
                            pts.append(m + R[:, 0] * t * math.sqrt(lam[0]))
                        elif i % 3 == 1:  # along the softest
                            pts.append(m + R[:, 2] * t * math.sqrt(lam[2]))
                        else:             # mixed, alternating signs: cancellation in s
                            pts.append(m + sum(R[:, a] * ((-1.0) ** (a + i // 3)) * t * math.sqrt(lam[a]) for a in range(3)))
                    yield mean, cov, np.array(pts)
    elif name == "offdiag":  # correlations of 0.9 .. 0.9999: strong off-diagonals, and the asymmetric 9 entries inv3 gives
        for _ in range(56):
            mean = rng.uniform(-2, 2, (6, 3))
            cov = []
            for _ in range(6):
                sd = 10.0 ** rng.uniform(-2, 0, 3)
                rho = (1.0 - 10.0 ** rng.uniform(-4, -1)) * rng.choice([-1.0, 1.0])
                a, b = int(rng.integers(0, 3)), int(rng.integers(1, 3))
                b = (a + b) % 3
                c = np.diag(sd * sd)
                c[a, b] = c[b, a] = rho * sd[a] * sd[b]
                cov.append(c)
            pts = [mean[i % 6] + rng.standard_normal(3) * 10.0 ** rng.uniform(-3, 0) for i in range(10)]
            yield mean, np.array(cov), np.array(pts)
    elif name == "far":  # the origin 1e3 .. 1e6 m from every mean (two clusters), and maps of extent 1e4: large R and rho
        for j in range(56):
            if j % 4 == 3:
                mean = rng.uniform(-5e3, 5e3, (6, 3))
            else:
                off = _unit(rng) * 10.0 ** rng.uniform(3, 6)
                mean = np.array([(off if i % 2 else -off) + rng.uniform(-1, 1, 3) for i in range(6)])
            cov = np.array([cov_of(10.0 ** rng.uniform(-4, 0, 3), quat_rot(rng)) for _ in range(6)])
            pts = [mean[i % 6] + rng.standard_normal(3) * 10.0 ** rng.uniform(-3, 0.5) for i in range(10)]
            yield mean, cov, np.array(pts)
    elif name == "near":  # on a mean, one fp64 ulp from it, and at distances that make D subnormal in fp32
        for _ in range(56):
            mean = rng.uniform(-1, 1, (6, 3))
            mean[0], mean[1], mean[2] = 0.0, 1.0, -1.0  # the origin is the middle of the extremes: component 0 is on it, so P - M can be subnormal
            cov = np.array([cov_of(10.0 ** rng.uniform(-6, 0, 3), quat_rot(rng)) for _ in range(6)])
            pts = [mean[i].copy() for i in range(3)]
            pts += [np.nextafter(mean[i], mean[i] + (1.0 if i % 2 else -1.0)) for i in range(3, 6)]
            pts += [mean[0] + _unit(rng) * 10.0 ** rng.uniform(-44, -38) for _ in range(3)]
            pts.append(mean[0] + _unit(rng) * 10.0 ** rng.uniform(-37, -10))
            yield mean, cov, np.array(pts)
    elif name == "gate":  # points up to the `ok` gate: big from 1e30 to 1e37
        for _ in range(56):
            mean = rng.uniform(-1, 1, (6, 3))
            cov = np.array([cov_of(10.0 ** rng.uniform(-6, 0, 3), quat_rot(rng)) for _ in range(6)])
            m = sm.ScreenMap(mean, cov)
            lo, hi = 1.0, 1e30  # the gate's radius along an axis, by bisection in the model
            for _ in range(120):
                mid = math.sqrt(lo * hi)
                lo, hi = (mid, hi) if sm.screen_point(m, (m.o[0] + mid, m.o[1], m.o[2])).ok else (lo, mid)
            pts = []
            for i in range(10):
                u = _unit(rng)
                u = u / np.abs(u).max()  # rho = |p - o|_inf decides
                pts.append(np.array(m.o) + u * lo * (1.0 - 1e-9) * (1.0 if i == 0 else 10.0 ** -rng.uniform(0, 2.4)))
            yield mean, cov, np.array(pts)
