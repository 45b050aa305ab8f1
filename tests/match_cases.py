"""Named scenes of a handful of features on both sides of the decisions the matcher kernels make, built by hand in numpy, for
tests/test_match_cases.py (CPU: the C++ oracle and oracle/numpy_ref.py both give the output each case declares) and
tests/test_gpu_match_cases.py (every case through every path of its kernel).  Test infrastructure.

Descriptors are ONE 256-bit word with exactly k chosen bits flipped (desc(k, at): the bits at .. at + k - 1), so the Hamming
distance of a candidate to a query holding the word itself is k: set, not drawn.  Every case declares the matcher, the decision
it sits on, its side, and the output it must give (the match array; the count is the number of its entries >= 0; for the fuse
search the best distances as well).  The decisions and the reference lines (DECISIONS below holds the same list for the
completeness check of the CPU test):

  searchByProjection, local map (orb_matcher.cpp:27-110)
    proj.th_high        :100  bestDist <= TH_HIGH (100)                                     100 / 101
    proj.ratio          :101  bestLevel == bestLevel2 && bestDist > nn_ratio * bestDist2    9/10, 10/11, 90/100, 91/100 at 0.9; 40/50, 41/50 at 0.8
    proj.ratio_level    :101  ... only when both are of one level                           10/11 with the second best an octave away
    proj.tie            :88-97  the first of equal distances in visiting order is the best  2 and 3 tied: one cell, two rows, two columns
    proj.viewcos        :49, :112-117  computeRadiusByViewingCos(float) > 0.998                      0.998, the doubles around float(0.998), the float below
    proj.u_right        :78-82  u_right > 0 and er > r                                      er == r, the float beyond; u_right -1, -0.0, 0.0, 1e-45
    proj.level_band     :54-56  getFeaturesInArea(.., lvl - 1, lvl)                           level 0 and 7, features an octave outside
    proj.taken          :74-76  a feature that has a map point on entry                       taken / free
    proj.invalid        :40-44  a map point that is not in view                               valid / not
  Frame::getFeaturesInArea / assignFeaturesToGrid (frame.cpp:54-79, :121-177), through searchByProjection
    grid.window_strict  :165  fabs(dist) < r                                                x + r and the float below, in x and y; a double that is no float
    grid.cell_round     :57-60  cell = round(u * inv)                                       512 x 384 (inv = 0.125): 20.0 (2.5), 508.0 (63.5), -4.0 (-0.5), v 380.0 (47.5)
    grid.window_clip    :127-150  the window cut at the image edge; empty window            near each edge, far outside on each side
  searchByProjection, last frame (orb_matcher.cpp:410-542)
    frame.direction     :425-426  tlc.z > mb / -tlc.z > mb, and not mono                    t.z = -/+ mb and the next double; mono
    frame.behind        :440  invzc < 0                                                     a point in front / behind
    frame.image         :448-451  u < 0, u > width (v alike)                                either side of u = 0 and of v = height, by bisection
    frame.level_window  :460-467  the level windows of the three directions                 octave 0 and 7
    frame.u_right       :485-490  u_right > 0 and er > radius, all in float                      er == radius and the float beyond; u_right -1, 0.0
    frame.th_high       :496, :502 bestDist <= TH_HIGH, the first of equal distances             100 / 101; tie
  rotation filter (orb_matcher.cpp:544-578), through searchByBoW, searchForTriangulation and the last-frame search
    rot.bin             :245-250, :365-370, :507-513  round(rot * factor), 30 -> 0, rot < 0 -> + 360      6, 30, 354, 359.9, a negative difference, -0.0
    rot.maxima          :544-578  three maxima, max2 < 0.1f * max1                          equal counts, 10/1, 20/2, 30/3 and 11/1, 21/2, 31/3; two bins; one match; off
  searchForTriangulation (orb_matcher.cpp:141-293, :119-139)
    tri.th_low          :219  dist > TH_LOW (50)                                            50 / 51
    tri.tie             :219  dist > bestDist: the LAST of equal distances that passes      two, three, three with the last failing the epipolar test
    tri.epipole         :224-230  both mono: distance to the epipole < 100 * sf[oct]        either side by bisection; a stereo side
    tri.epipolar        :119-139  dsqr < 3.84 * sigma2[oct]                                 either side by bisection, octave 0 and 7
    tri.den             :133  den == 0                                                      a matrix whose line is a = b = 0
    tri.stereo          :188-192, :209-213  u_right >= 0; only_stereo                               -0.0, 0.0, -1
    tri.has_mp          :183-186, :204-207  a feature with a map point, on either key-frame         one each
  searchByBoW (orb_matcher.cpp:295-408)
    bow.th_low          :357  bestDist1 <= TH_LOW                                           50 / 51
    bow.ratio           :358-359 (float)b1 < nn_ratio * (float)b2                              4/5, 3/5, 40/50, 39/50 at 0.8; 3/5, 2/5 at 0.6; one partner
    bow.tie             :348-354  a later equal distance becomes the second best            tie: rejected
    bow.reject_claims_nothing  :357-360  a query that rejects leaves the feature free       the next query of the node takes it
    bow.node            :316-317, :381-386  node shared by both / not; empty list                     one each
    bow.has_mp          :324-330  a key-frame feature without a valid map point             one
  fuse search (localization.cpp:226-318)
    fuse.th_low         :304  best_dist <= TH_LOW, the first minimum in visiting order      50 / 51; tie across two cells
    fuse.chi2           :281-296  err > 5.99 (mono) / > 7.8 (stereo), scaled by the level   either side by bisection, octave 0 and 3; u_right -1 / -0.0 / 0.0
    fuse.level_band     :262  getFeaturesInArea(.., lvl - 1, lvl)                           level 0 and 7

The regime scenes (wide_window, conflict_chain, deep_chain, big_node) are the smallest scenes on which a kernel leaves its common path; they declare no output by hand (it
is the oracle's, bit for bit) but a property of it that shows the regime was entered."""
import numpy as np

from gmmloc_amd import api
from oracle import numpy_ref

f32, f64 = np.float32, np.float64
BASE = np.random.default_rng(20240607).integers(0, 256, 32, dtype=np.uint8)
W0, H0 = 752, 480      # the reference's image (cell 11.75 x 10)
WG, HG = 512, 384      # both inverse cell sizes are 0.125
CAM = api.Camera()
MB = f64(f32(f32(CAM.bf) / f32(CAM.fx)))  # frame.cpp:24, as the kernel forms it

DECISIONS = {
    "proj.th_high": "orb_matcher.cpp:100", "proj.ratio": "orb_matcher.cpp:101", "proj.ratio_level": "orb_matcher.cpp:101",
    "proj.tie": "orb_matcher.cpp:88-97", "proj.viewcos": "orb_matcher.cpp:49", "proj.u_right": "orb_matcher.cpp:78-82",
    "proj.level_band": "orb_matcher.cpp:54-56", "proj.taken": "orb_matcher.cpp:74-76", "proj.invalid": "orb_matcher.cpp:40-44",
    "grid.window_strict": "frame.cpp:165", "grid.cell_round": "frame.cpp:57-60", "grid.window_clip": "frame.cpp:127-150",
    "frame.direction": "orb_matcher.cpp:425-426", "frame.behind": "orb_matcher.cpp:440", "frame.image": "orb_matcher.cpp:448-451",
    "frame.level_window": "orb_matcher.cpp:460-467", "frame.u_right": "orb_matcher.cpp:485-490", "frame.th_high": "orb_matcher.cpp:502",
    "rot.bin": "orb_matcher.cpp:365-370", "rot.maxima": "orb_matcher.cpp:544-578",
    "tri.th_low": "orb_matcher.cpp:219", "tri.tie": "orb_matcher.cpp:219", "tri.epipole": "orb_matcher.cpp:224-230",
    "tri.epipolar": "orb_matcher.cpp:119-139", "tri.den": "orb_matcher.cpp:133", "tri.stereo": "orb_matcher.cpp:188-192",
    "tri.has_mp": "orb_matcher.cpp:183-186",
    "bow.th_low": "orb_matcher.cpp:357", "bow.ratio": "orb_matcher.cpp:358-359", "bow.tie": "orb_matcher.cpp:348-354",
    "bow.reject_claims_nothing": "orb_matcher.cpp:357-360", "bow.node": "orb_matcher.cpp:316-317", "bow.has_mp": "orb_matcher.cpp:324-330",
    "fuse.th_low": "localization.cpp:304", "fuse.chi2": "localization.cpp:281-296", "fuse.level_band": "localization.cpp:262",
}


def desc(k, at=0):
    """BASE with the k bits at .. at + k - 1 flipped"""
    d = BASE.copy()
    bits = (at + np.arange(k)) % 256
    np.bitwise_xor.at(d, bits // 8, (1 << (bits % 8)).astype(np.uint8))
    return d


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def below(x):
    return np.nextafter(x, type(x)(-np.inf))


def above(x):
    return np.nextafter(x, type(x)(np.inf))


# ---- one feature / query, and the scenes made of them ------------------------------------------------------------------------
def F(u, v, k=0, oct=0, ur=-1.0, taken=0, at=0, angle=0.0, has_mp=0):
    return dict(u=u, v=v, k=k, oct=oct, ur=ur, taken=taken, at=at, angle=angle, has_mp=has_mp)


def Q(x, y, ur=0.0, lvl=0, cos=0.5, valid=1, k=0, at=0):
    return dict(x=x, y=y, ur=ur, lvl=lvl, cos=cos, valid=valid, k=k, at=at)


def _feat_arrays(feats):
    return dict(feat_uv=np.array([[f["u"], f["v"]] for f in feats], f64).reshape(-1, 2), feat_ur=np.array([f["ur"] for f in feats], f32),
                feat_oct=np.array([f["oct"] for f in feats], np.int32), feat_desc=np.stack([desc(f["k"], f["at"]) for f in feats]))


def proj_scene(feats, qs, size=(W0, H0)):
    """the inputs of searchByProjection (local map) / the fuse search: tests/test_gpu_match.py KEYS / FUSE_KEYS"""
    s = dict(width=size[0], height=size[1], **_feat_arrays(feats))
    s["feat_taken"] = np.array([f["taken"] for f in feats], np.uint8)
    s["mp_uvr"] = np.array([[q["x"], q["y"], q["ur"]] for q in qs], f64)
    s["mp_level"] = np.array([q["lvl"] for q in qs], f64)
    s["mp_viewcos"] = np.array([q["cos"] for q in qs], f64)
    s["mp_valid"] = np.array([q["valid"] for q in qs], np.uint8)
    s["mp_desc"] = np.stack([desc(q["k"], q["at"]) for q in qs])
    return s


def frame_scene(feats, pts, tz=0.0, ptz=5.0):
    """the inputs of searchByProjection (last frame), tests/test_gpu_match.py FKEYS: both rotations the identity, the current camera
    at z = -tz of the last one (tlc.z = -tz), the last frame's points given by the pixel they project to (or as x, y, z in the
    CURRENT camera under "ptc"), ptz in front"""
    s = _feat_arrays(feats)
    s["feat_angle"] = np.array([f["angle"] for f in feats], f32)
    s["feat_taken"] = np.array([f["taken"] for f in feats], np.uint8)
    s["pose_cw"] = np.array([0, 0, 0, 1, 0, 0, tz], f64)
    s["pose_lw"] = np.array([0, 0, 0, 1, 0, 0, 0], f64)
    P = []
    for p in pts:
        if "ptc" in p:
            c = np.array(p["ptc"], f64)
        else:
            c = np.array([(p["x"] - f64(f32(CAM.cx))) / f64(f32(CAM.fx)) * ptz, (p["y"] - f64(f32(CAM.cy))) / f64(f32(CAM.fy)) * ptz, ptz])
        P.append(c - s["pose_cw"][4:])
    s["last_pt"] = np.array(P, f64).reshape(-1, 3)
    s["last_valid"] = np.array([p.get("valid", 1) for p in pts], np.uint8)
    s["last_oct"] = np.array([p.get("oct", 0) for p in pts], np.int32)
    s["last_angle"] = np.array([p.get("angle", 0.0) for p in pts], f32)
    s["last_desc"] = np.stack([desc(p.get("k", 0), p.get("at", 0)) for p in pts])
    return s


def L(x, y, **kw):
    return dict(x=x, y=y, **kw)


def kf_side(feats, nodes):
    """one key-frame of searchForTriangulation / searchByBoW: the features and the DBoW2 feature vector {node id: [features]} as CSR"""
    a = _feat_arrays(feats)
    ids = sorted(nodes)
    ptr = np.cumsum([0] + [len(nodes[i]) for i in ids]).astype(np.int32)
    idx = np.array([j for i in ids for j in nodes[i]], np.int32)
    return dict(uv=a["feat_uv"], ur=a["feat_ur"], oct=a["feat_oct"], angle=np.array([f["angle"] for f in feats], f32), desc=a["feat_desc"],
                has_mp=np.array([f["has_mp"] for f in feats], np.uint8), node_id=np.array(ids, np.int32), node_ptr=ptr, node_idx=idx)


F_ROWS = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f64)  # the line of (u1, v1) is v2 = v1, den = 1: dsqr = (v2 - v1) ^ 2
FAR = np.array([-1e4, -1e4], f32)                           # an epipole nowhere near


def tri_scene(f1, f2, nodes1=None, nodes2=None, fmat=F_ROWS, epipole=FAR):
    n1 = nodes1 if nodes1 is not None else {0: list(range(len(f1)))}
    n2 = nodes2 if nodes2 is not None else {0: list(range(len(f2)))}
    return dict(kf1=kf_side(f1, n1), kf2=kf_side(f2, n2), fmat=np.array(fmat, f64), epipole=np.array(epipole, f32))


def bow_scene(fk, ff, nodes1=None, nodes2=None):
    n1 = nodes1 if nodes1 is not None else {0: list(range(len(fk)))}
    n2 = nodes2 if nodes2 is not None else {0: list(range(len(ff)))}
    return (kf_side(fk, n1), kf_side(ff, n2))


# ---- running a case on the oracle or on numpy_ref (the same function names and arguments) --------------------------------------------
FUSE_KEYS = ("feat_uv", "feat_ur", "feat_oct", "feat_desc", "mp_uvr", "mp_level", "mp_valid", "mp_desc")


def run(impl, matcher, data, kw):
    """-> (match, count, best_dist or None)"""
    if matcher == "proj":
        m, n = impl.search_by_projection(**data, **kw)
    elif matcher == "frame":
        m, n = impl.search_by_projection_frame(CAM, **data, **kw)
    elif matcher == "tri":
        m, n = impl.search_for_triangulation(data["kf1"], data["kf2"], data["fmat"], data["epipole"], **kw)
    elif matcher == "bow":
        m, n = impl.search_by_bow(data[0], data[1], **kw)
    else:
        bi, bd, n = impl.fuse_search(data["width"], data["height"], *[data[k] for k in FUSE_KEYS], **kw)
        return bi, n, bd
    return m, n, None


class Case:
    def __init__(self, name, matcher, decision, side, data, want, kw, dist=None):
        assert decision in DECISIONS, decision
        self.name, self.matcher, self.decision, self.side, self.data, self.kw = name, matcher, decision, side, data, kw
        self.want = np.array(want, np.int32)
        self.n = int((self.want >= 0).sum())
        self.dist = None if dist is None else np.array(dist, np.int32)
        self.size = (data["width"], data["height"]) if isinstance(data, dict) and "width" in data else (W0, H0)


CASES = {}
PAIRS = []  # (case, case, the element of the output in which the two differ)


def add(name, matcher, decision, side, data, want, dist=None, **kw):
    assert name not in CASES, name
    CASES[name] = Case(name, matcher, decision, side, data, want, kw, dist)
    return name


def pair(a, b, elem=0):
    PAIRS.append((a, b, elem))


def bisect(decide, lo, hi):
    """lo, hi: two values of one scalar input (np.float32 or np.float64) on which decide(x) differs -> the adjacent representable
    values (a, b), a on lo's side, with decide(a) == decide(lo) != decide(b)"""
    t = type(lo)
    assert t in (f32, f64) and type(hi) is t
    dl, dh = decide(lo), decide(hi)
    assert dl != dh, "the two ends decide alike"
    while True:
        mid = t(lo / 2 + hi / 2)
        if mid == lo or mid == hi:
            break
        if decide(mid) == dl:
            lo = mid
        else:
            hi = mid
    assert np.nextafter(lo, hi) == hi and decide(lo) == dl and decide(hi) == dh
    return lo, hi


def outcome(matcher, data, kw):
    m, n, d = run(numpy_ref, matcher, data, kw)
    return tuple(m.tolist())


# ================================================ searchByProjection, local map ====================================================
X0, Y0 = 300.0, 200.0  # cell (26, 20) of the 752 x 480 grid; th = 3: a window of 12 (4.0 x 3) at level 0


def _p(name, decision, side, feats, qs, want, th=3.0, nn_ratio=0.8, size=(W0, H0)):
    return add(name, "proj", decision, side, proj_scene(feats, qs, size), want, th=th, nn_ratio=nn_ratio)


pair(_p("proj_best_100", "proj.th_high", "accepted", [F(X0, Y0, 100)], [Q(X0, Y0)], [0]),
     _p("proj_best_101", "proj.th_high", "rejected", [F(X0, Y0, 101)], [Q(X0, Y0)], [-1]))
for _b, _b2, _r, _ok in ((9, 10, 0.9, 1), (10, 11, 0.9, 0), (90, 100, 0.9, 1), (91, 100, 0.9, 0), (40, 50, 0.8, 1), (41, 50, 0.8, 0), (45, 50, 0.9, 1)):
    _p("proj_ratio_%d_%d_at_%g" % (_b, _b2, _r), "proj.ratio", "accepted" if _ok else "rejected",
       [F(X0, Y0, _b), F(X0 + 2, Y0, _b2, at=128)], [Q(X0, Y0)], [0 if _ok else -1, -1], nn_ratio=_r)
pair("proj_ratio_90_100_at_0.9", "proj_ratio_91_100_at_0.9")
pair("proj_ratio_40_50_at_0.8", "proj_ratio_41_50_at_0.8")
pair(_p("proj_ratio_other_level", "proj.ratio_level", "levels differ", [F(X0, Y0, 10, oct=1), F(X0 + 2, Y0, 11, oct=0, at=128)], [Q(X0, Y0, lvl=1)], [0, -1], nn_ratio=0.9),
     _p("proj_ratio_same_level", "proj.ratio_level", "levels equal", [F(X0, Y0, 10, oct=1), F(X0 + 2, Y0, 11, oct=1, at=128)], [Q(X0, Y0, lvl=1)], [-1, -1], nn_ratio=0.9))
# ties (nn_ratio above 1: the ratio test is off).  u = 293 is column 25, u = 300 column 26; v = 194 row 19, v = 200 row 20.
_p("proj_tie2_one_cell", "proj.tie", "one cell: the lower index", [F(X0, Y0, 20), F(X0 + 1, Y0, 20, at=128)], [Q(X0, Y0)], [0, -1], nn_ratio=1.1)
_p("proj_tie2_two_rows", "proj.tie", "two rows: the upper cell", [F(X0, Y0, 20), F(X0, 194.0, 20, at=128)], [Q(X0, Y0)], [-1, 0], nn_ratio=1.1)
_p("proj_tie2_two_columns", "proj.tie", "two columns: the left cell", [F(X0, 194.0, 20), F(293.0, Y0, 20, at=128)], [Q(X0, Y0)], [-1, 0], nn_ratio=1.1)
_p("proj_tie3_one_cell", "proj.tie", "three in one cell", [F(X0, Y0, 21), F(X0 + 1, Y0, 20, at=64), F(X0 + 2, Y0, 20, at=128)], [Q(X0, Y0)], [-1, 0, -1], nn_ratio=1.1)
_p("proj_tie3_rows_columns", "proj.tie", "three: column before row before index",
   [F(X0, Y0, 20), F(X0, 194.0, 20, at=64), F(293.0, Y0, 20, at=128)], [Q(X0, Y0)], [-1, -1, 0], nn_ratio=1.1)
_p("proj_tie_is_second_best", "proj.tie", "a later equal distance is the second best: the ratio test fails",
   [F(X0, Y0, 20), F(X0 + 1, Y0, 20, at=128)], [Q(X0, Y0)], [-1, -1], nn_ratio=0.8)
# viewing cosine: a feature 10 px away is inside the 4.0 x 3 window and outside the 2.5 x 3 one
_C = f64(f32(0.998))
for _n, _c, _wide in (("0.998_as_double", 0.998, 0), ("float_0.998", _C, 0), ("double_below_float_0.998", below(_C), 0), ("double_above_float_0.998", above(_C), 0),
                      ("float_below_0.998", f64(below(f32(0.998))), 1), ("0.9979", 0.9979, 1)):
    _p("proj_viewcos_" + _n, "proj.viewcos", "4.0" if _wide else "2.5", [F(X0 + 10, Y0, 5)], [Q(X0, Y0, cos=_c)], [0 if _wide else -1])
pair("proj_viewcos_float_0.998", "proj_viewcos_float_below_0.998")
# u_right: the query's is 250, the window 12
for _n, _ur, _ok in (("er_equals_r", f32(238.0), 1), ("er_float_above_r", below(f32(238.0)), 0), ("minus_1", f32(-1.0), 1), ("minus_0", f32(-0.0), 1),
                     ("plus_0", f32(0.0), 1), ("smallest_positive", f32(1e-45), 0)):
    _p("proj_ur_" + _n, "proj.u_right", "passes" if _ok else "fails", [F(X0, Y0, 5, ur=_ur)], [Q(X0, Y0, ur=250.0)], [0 if _ok else -1])
pair("proj_ur_er_equals_r", "proj_ur_er_float_above_r")
pair("proj_ur_plus_0", "proj_ur_smallest_positive")
for _lvl in (0, 7):
    for _o, _ok in ((_lvl - 2, 0), (_lvl - 1, 1), (_lvl, 1), (_lvl + 1, 0)):
        if 0 <= _o <= 7:
            _p("proj_level_%d_octave_%d" % (_lvl, _o), "proj.level_band", "inside" if _ok else "outside", [F(X0, Y0, 5, oct=_o)], [Q(X0, Y0, lvl=_lvl)], [0 if _ok else -1])
pair("proj_level_0_octave_0", "proj_level_0_octave_1")
pair("proj_level_7_octave_5", "proj_level_7_octave_6")
pair(_p("proj_taken_on_entry", "proj.taken", "taken", [F(X0, Y0, 5, taken=1), F(X0 + 1, Y0, 30, at=128)], [Q(X0, Y0)], [-1, 0]),
     _p("proj_not_taken", "proj.taken", "free", [F(X0, Y0, 5), F(X0 + 1, Y0, 30, at=128)], [Q(X0, Y0)], [0, -1]))
pair(_p("proj_invalid_point", "proj.invalid", "invalid", [F(X0, Y0, 5)], [Q(X0, Y0, valid=0), Q(X0 + 1, Y0, k=3, at=200)], [1]),
     _p("proj_valid_point", "proj.invalid", "valid", [F(X0, Y0, 5)], [Q(X0, Y0), Q(X0 + 1, Y0, k=3, at=200)], [0]))

# ================================================ the grid, through searchByProjection ================================================
# 512 x 384, th = 1 (no factor): a window of exactly 4.0 at level 0
def _g(name, decision, side, feats, qs, want, nn_ratio=0.8):
    return _p(name, decision, side, feats, qs, want, th=1.0, nn_ratio=nn_ratio, size=(WG, HG))


pair(_g("grid_x_plus_r", "grid.window_strict", "outside", [F(104.0, 100.0, 5)], [Q(100.0, 100.0)], [-1]),
     _g("grid_x_plus_r_float_below", "grid.window_strict", "inside", [F(f64(below(f32(104.0))), 100.0, 5)], [Q(100.0, 100.0)], [0]))
pair(_g("grid_y_plus_r", "grid.window_strict", "outside", [F(100.0, 104.0, 5)], [Q(100.0, 100.0)], [-1]),
     _g("grid_y_plus_r_float_below", "grid.window_strict", "inside", [F(100.0, f64(below(f32(104.0))), 5)], [Q(100.0, 100.0)], [0]))
_g("grid_x_minus_r", "grid.window_strict", "outside", [F(96.0, 100.0, 5)], [Q(100.0, 100.0)], [-1])
# a double that is not a float (the general walk): the difference is rounded to float BEFORE it is compared, so 104 - 1e-9 is
# still outside (the difference rounds to 4.0f) and 104 - 3e-7 is inside (3.9999998f)
pair(_g("grid_x_plus_r_double_1e-9_below", "grid.window_strict", "outside", [F(104.0 - 1e-9, 100.0, 5)], [Q(100.0, 100.0)], [-1]),
     _g("grid_x_plus_r_double_3e-7_below", "grid.window_strict", "inside", [F(104.0 - 3e-7, 100.0, 5)], [Q(100.0, 100.0)], [0]))
pair(_g("grid_y_plus_r_double_1e-9_below", "grid.window_strict", "outside", [F(100.0, 104.0 - 1e-9, 5)], [Q(100.0, 100.0)], [-1]),
     _g("grid_y_plus_r_double_3e-7_below", "grid.window_strict", "inside", [F(100.0, 104.0 - 3e-7, 5)], [Q(100.0, 100.0)], [0]))
# cell by round: u = 20.0 is 2.5 -> column 3 (half-even: 2).  A tie: feature 0 at u = 20.0, feature 1 at u = 17.0 (column 2): feature
# 1 is visited first.  Were 20.0 put in column 2, feature 0 (the lower index of one cell) would be.
pair(_g("grid_tie_u_20", "grid.cell_round", "k + 0.5 rounds up: the other column first", [F(20.0, 100.0, 20), F(17.0, 100.0, 20, at=128)], [Q(18.0, 100.0)], [-1, 0], nn_ratio=1.1),
     _g("grid_tie_u_float_below_20", "grid.cell_round", "below k + 0.5: one cell, the lower index", [F(f64(below(f32(20.0))), 100.0, 20), F(17.0, 100.0, 20, at=128)],
        [Q(18.0, 100.0)], [0, -1], nn_ratio=1.1))
pair(_g("grid_tie_v_20", "grid.cell_round", "k + 0.5 rounds up: the other row first", [F(100.0, 20.0, 20), F(100.0, 17.0, 20, at=128)], [Q(100.0, 18.0)], [-1, 0], nn_ratio=1.1),
     _g("grid_tie_v_float_below_20", "grid.cell_round", "below k + 0.5: one cell, the lower index", [F(100.0, f64(below(f32(20.0))), 20), F(100.0, 17.0, 20, at=128)],
        [Q(100.0, 18.0)], [0, -1], nn_ratio=1.1))
pair(_g("grid_u_508", "grid.cell_round", "63.5 -> 64: not in the grid", [F(508.0, 100.0, 5)], [Q(506.0, 100.0)], [-1]),
     _g("grid_u_float_below_508", "grid.cell_round", "column 63", [F(f64(below(f32(508.0))), 100.0, 5)], [Q(506.0, 100.0)], [0]))
pair(_g("grid_u_minus_4", "grid.cell_round", "-0.5 -> -1: not in the grid", [F(-4.0, 100.0, 5)], [Q(-2.0, 100.0)], [-1]),
     _g("grid_u_float_above_minus_4", "grid.cell_round", "column 0", [F(f64(above(f32(-4.0))), 100.0, 5)], [Q(-2.0, 100.0)], [0]))
pair(_g("grid_v_380", "grid.cell_round", "47.5 -> 48: not in the grid", [F(100.0, 380.0, 5)], [Q(100.0, 378.0)], [-1]),
     _g("grid_v_float_below_380", "grid.cell_round", "row 47", [F(100.0, f64(below(f32(380.0))), 5)], [Q(100.0, 378.0)], [0]))
pair(_g("grid_v_minus_4", "grid.cell_round", "-0.5 -> -1: not in the grid", [F(100.0, -4.0, 5)], [Q(100.0, -2.0)], [-1]),
     _g("grid_v_float_above_minus_4", "grid.cell_round", "row 0", [F(100.0, f64(above(f32(-4.0))), 5)], [Q(100.0, -2.0)], [0]))
# the window at the image edge (the feature 3 px inside of the query) and far outside (nothing to visit)
for _n, _q, _f in (("left", (-2.0, 100.0), (1.0, 100.0)), ("right", (510.0, 100.0), (507.0, 100.0)), ("top", (100.0, -2.0), (100.0, 1.0)),
                   ("bottom", (100.0, 382.0), (100.0, 379.0))):
    _g("grid_edge_" + _n, "grid.window_clip", "clipped", [F(*_f, 5)], [Q(*_q)], [0])
for _n, _q in (("left", (-100.0, 100.0)), ("right", (700.0, 100.0)), ("top", (100.0, -100.0)), ("bottom", (100.0, 600.0))):
    _g("grid_far_" + _n, "grid.window_clip", "empty", [F(1.0, 1.0, 5), F(507.0, 379.0, 5, at=128)], [Q(*_q)], [-1, -1])

# ================================================ searchByProjection, last frame =====================================================
# the point projects to (cx, cy); th = 7: a window of 7 at octave 0
CX, CY = f64(f32(CAM.cx)), f64(f32(CAM.cy))
FX0, FY0 = 367.0, 252.0  # a feature half a pixel from (cx, cy)


def _f(name, decision, side, feats, pts, want, tz=0.0, th=7.0, mono=False, chk=False, ptz=5.0):
    return add(name, "frame", decision, side, frame_scene(feats, pts, tz, ptz), want, th=th, mono=mono, check_orientation=chk)


_PT = dict(ptc=(0.0, 0.0, 5.0))
# forward (tlc.z > mb): levels oct .. ; a feature one octave BELOW the point's shows which
pair(_f("frame_tz_mb", "frame.direction", "not forward", [F(FX0, FY0, 5, oct=2)], [dict(_PT, oct=3)], [0], tz=-MB),
     _f("frame_tz_above_mb", "frame.direction", "forward", [F(FX0, FY0, 5, oct=2)], [dict(_PT, oct=3)], [-1], tz=-above(MB)))
# backward (-tlc.z > mb): levels 0 .. oct; a feature one octave ABOVE
pair(_f("frame_tz_minus_mb", "frame.direction", "not backward", [F(FX0, FY0, 5, oct=4)], [dict(_PT, oct=3)], [0], tz=MB),
     _f("frame_tz_below_minus_mb", "frame.direction", "backward", [F(FX0, FY0, 5, oct=4)], [dict(_PT, oct=3)], [-1], tz=above(MB)))
_f("frame_forward_mono", "frame.direction", "mono: never forward", [F(FX0, FY0, 5, oct=2)], [dict(_PT, oct=3)], [0], tz=-1.0, mono=True)
_f("frame_backward_mono", "frame.direction", "mono: never backward", [F(FX0, FY0, 5, oct=4)], [dict(_PT, oct=3)], [0], tz=1.0, mono=True)
pair(_f("frame_point_in_front", "frame.behind", "in front", [F(FX0, FY0, 5)], [dict(ptc=(0.0, 0.0, 5.0))], [0]),
     _f("frame_point_behind", "frame.behind", "behind", [F(FX0, FY0, 5)], [dict(ptc=(0.0, 0.0, -5.0))], [-1]))


BISECTED = {}  # name of a bisected pair -> the two adjacent values


def _bisect_frame(name, axis, lo, hi, feat, sides):
    """either side of an image border: the point's x (or y) in the camera, bisected over the doubles"""
    def scene(t):
        c = [0.0, 0.0, 5.0]
        c[axis] = float(t)
        return frame_scene([F(*feat, 5)], [dict(ptc=tuple(c))], 0.0)
    kw = dict(th=7.0, mono=False, check_orientation=False)
    a, b = bisect(lambda t: outcome("frame", scene(t), kw), f64(lo), f64(hi))
    na = add(name + "_" + sides[0].replace(" ", "_"), "frame", "frame.image", sides[0], scene(a), [0], **kw)
    nb = add(name + "_" + sides[1].replace(" ", "_"), "frame", "frame.image", sides[1], scene(b), [-1], **kw)
    BISECTED[name] = (a, b)
    pair(na, nb)


# u = 0 sits at x = -cx / fx * z; the feature 2 px inside the image: matched on the inside, and on the outside NOT although it is in the window
_bisect_frame("frame_u_0", 0, -CX / f64(f32(CAM.fx)) * 5.0 + 0.02, -CX / f64(f32(CAM.fx)) * 5.0 - 0.02, (2.0, FY0), ("inside", "u below 0"))
_bisect_frame("frame_v_height", 1, (480.0 - CY) / f64(f32(CAM.fy)) * 5.0 - 0.02, (480.0 - CY) / f64(f32(CAM.fy)) * 5.0 + 0.02, (FX0, 474.0), ("inside", "v above height"))
_bisect_frame("frame_u_width", 0, (752.0 - CX) / f64(f32(CAM.fx)) * 5.0 - 0.02, (752.0 - CX) / f64(f32(CAM.fx)) * 5.0 + 0.02, (746.0, FY0), ("inside", "u above width"))
_bisect_frame("frame_v_0", 1, -CY / f64(f32(CAM.fy)) * 5.0 + 0.02, -CY / f64(f32(CAM.fy)) * 5.0 - 0.02, (FX0, 2.0), ("inside", "v below 0"))
# the level windows: no direction oct - 1 .. oct + 1, forward oct .., backward 0 .. oct
for _dir, _tz in (("none", 0.0), ("forward", -1.0), ("backward", 1.0)):
    for _o in (0, 7):
        lo, hi = {"none": (_o - 1, _o + 1), "forward": (_o, 7), "backward": (0, _o)}[_dir]
        for _fo in sorted({0, 1, 2, 5, 6, 7}):
            if _dir == "none" and abs(_fo - _o) > 2:
                continue
            _ok = lo <= _fo <= hi
            _f("frame_%s_oct_%d_feature_%d" % (_dir, _o, _fo), "frame.level_window", "inside" if _ok else "outside", [F(FX0, FY0, 5, oct=_fo)], [dict(_PT, oct=_o)],
               [0 if _ok else -1], tz=_tz)
pair(_f("frame_best_100", "frame.th_high", "accepted", [F(FX0, FY0, 100)], [_PT], [0]),
     _f("frame_best_101", "frame.th_high", "rejected", [F(FX0, FY0, 101)], [_PT], [-1]))
# u_right of the point: u - mbf * invzc in float (u = cx, z = 5); a feature's 7.0 below it is exactly the radius away
_URF = f32(f32(CAM.cx) - f32(f32(CAM.bf) * f32(1.0 / 5.0)))
assert f32(_URF - f32(_URF - f32(7.0))) == f32(7.0)
for _n, _ur, _ok in (("er_equals_radius", f32(_URF - f32(7.0)), 1), ("er_float_above_radius", below(f32(_URF - f32(7.0))), 0), ("minus_1", f32(-1.0), 1), ("zero", f32(0.0), 1),
                     ("far", f32(100.0), 0)):
    _f("frame_ur_" + _n, "frame.u_right", "passes" if _ok else "fails", [F(FX0, FY0, 5, ur=_ur)], [_PT], [0 if _ok else -1])
pair("frame_ur_er_equals_radius", "frame_ur_er_float_above_radius")
_f("frame_tie_first_wins", "frame.th_high", "tie: the first in visiting order", [F(FX0, FY0, 20), F(FX0 + 1, FY0, 20, at=128), F(FX0 - 10, FY0, 20, at=64)], [_PT], [0, -1, -1])

# ================================================ the rotation filter =================================================================
# One match per entry of `rots` = (angle of the query side, angle of the other side): rot = a1 - a2.  Built for each of the three
# matchers that have the filter; match i is query i <-> partner i (descriptor desc(0, 8 i) on both sides, 16 bits from every other).
def rot_scene(matcher, rots):
    n = len(rots)
    assert n <= 40
    if matcher == "bow":  # match21[frame feature i] = key-frame feature i
        fk = [F(0, 0, 16, at=6 * i, angle=a1, has_mp=1) for i, (a1, a2) in enumerate(rots)]
        ff = [F(0, 0, 16, at=6 * i, angle=a2) for i, (a1, a2) in enumerate(rots)]
        return bow_scene(fk, ff), dict(nn_ratio=0.7)
    if matcher == "tri":  # features on a row each (v = 10 i): only partner i passes the epipolar test
        f1 = [F(100.0, 10.0 * i, 16, at=6 * i, angle=a1) for i, (a1, a2) in enumerate(rots)]
        f2 = [F(120.0, 10.0 * i, 16, at=6 * i, angle=a2) for i, (a1, a2) in enumerate(rots)]
        return tri_scene(f1, f2), dict(only_stereo=False)
    # last frame: point i projects onto feature i, 40 px apart (match[feature i] = i)
    xy = [(60.0 + 80.0 * (i % 8), 60.0 + 80.0 * (i // 8)) for i in range(n)]
    feats = [F(x, y, 16, at=6 * i, angle=a2) for i, ((a1, a2), (x, y)) in enumerate(zip(rots, xy))]
    pts = [L(x + 0.25, y + 0.25, k=16, at=6 * i, angle=a1) for i, ((a1, a2), (x, y)) in enumerate(zip(rots, xy))]
    return frame_scene(feats, pts), dict(th=7.0, mono=False)


def _r(name, decision, side, rots, kept, matchers=("bow", "tri", "frame"), chk=True):
    want = [i if k else -1 for i, k in enumerate(kept)]
    for m in matchers:
        data, kw = rot_scene(m, rots)
        add("rot_%s_%s" % (name, m), m, decision, side, data, want, check_orientation=chk, **kw)


def _probe(a1, a2, target):
    """three matches in bin 10, three in bin 20, two in the middle of bin `target`, and the probe (a1, a2): kept iff its bin is `target`
    (elsewhere it is a fourth bin of one match)"""
    return [(120.0, 0.0)] * 3 + [(240.0, 0.0)] * 3 + [(12.0 * target, 0.0)] * 2 + [(a1, a2)]


ROT_FACTOR = f32(f32(30) / f32(360.0))  # orb_matcher.cpp:171, :308, :417


def first_float_rounding_below(rot):
    """the largest float below `rot` (a float whose rot * factor is k + 0.5) whose product, rounded to float as the reference forms it, is
    below k + 0.5: NOT the float next to rot - the product of that one still rounds to k + 0.5"""
    half, x = f32(f32(rot) * ROT_FACTOR), f32(rot)
    while f32(x * ROT_FACTOR) >= half:
        x = below(x)
    return x


_K8 = [1] * 8
for _n, _a, _t, _in in (("6", (6.0, 0.0), 1, 1), ("below_6", (float(first_float_rounding_below(6.0)), 0.0), 1, 0), ("30", (30.0, 0.0), 3, 1),
                        ("float_below_30", (float(below(f32(30.0))), 0.0), 3, 1), ("below_30", (float(first_float_rounding_below(30.0)), 0.0), 3, 0),
                        ("354", (354.0, 0.0), 0, 1), ("below_354", (float(first_float_rounding_below(354.0)), 0.0), 0, 0), ("359.9", (359.9, 0.0), 0, 1),
                        ("negative", (10.0, 16.0), 0, 1), ("negative_one_bin_on", (10.0, 28.0), 0, 0), ("minus_0", (-0.0, 0.0), 0, 1)):
    _r("bin_" + _n, "rot.bin", "in bin %d" % _t if _in else "not in bin %d" % _t, _probe(*_a, _t), _K8 + [_in])


def _counts(c):
    """{bin: matches} -> rots, in the middle of their bins"""
    return [(12.0 * b, 0.0) for b, n in c.items() for _ in range(n)]


_r("equal_counts", "rot.maxima", "four equal bins: the first three", _counts({5: 2, 6: 2, 7: 2, 8: 2}), [1] * 6 + [0] * 2)
for _m1, _m2 in ((10, 1), (20, 2), (30, 3)):
    _r("%d_%d" % (_m1, _m2), "rot.maxima", "second kept", _counts({4: _m1, 9: _m2}), [1] * (_m1 + _m2))
    _r("%d_%d" % (_m1 + 1, _m2), "rot.maxima", "second dropped", _counts({4: _m1 + 1, 9: _m2}), [1] * (_m1 + 1) + [0] * _m2)
_r("10_1_1", "rot.maxima", "third kept", _counts({4: 10, 9: 1, 15: 1}), [1] * 12)
_r("10_2_1", "rot.maxima", "third kept", _counts({4: 10, 9: 2, 15: 1}), [1] * 13)
_r("11_2_1", "rot.maxima", "third dropped", _counts({4: 11, 9: 2, 15: 1}), [1] * 13 + [0])
_r("two_bins", "rot.maxima", "two bins", _counts({4: 3, 9: 2}), [1] * 5)
_r("one_match", "rot.maxima", "one match", _counts({4: 1}), [1])
_r("off", "rot.maxima", "check_orientation off", _counts({5: 2, 6: 2, 7: 2, 8: 2}), [1] * 8, chk=False)
pair("rot_bin_30_bow", "rot_bin_below_30_bow", 8)
pair("rot_bin_30_tri", "rot_bin_below_30_tri", 8)
pair("rot_bin_30_frame", "rot_bin_below_30_frame", 8)
pair("rot_bin_6_bow", "rot_bin_below_6_bow", 8)
pair("rot_bin_354_bow", "rot_bin_below_354_bow", 8)
pair("rot_equal_counts_bow", "rot_off_bow", 6)

# ================================================ searchForTriangulation ==========================================================
def _t(name, decision, side, f1, f2, want, only_stereo=False, chk=False, **sc):
    return add(name, "tri", decision, side, tri_scene(f1, f2, **sc), want, only_stereo=only_stereo, check_orientation=chk)


pair(_t("tri_dist_50", "tri.th_low", "accepted", [F(100.0, 50.0)], [F(120.0, 50.0, 50)], [0]),
     _t("tri_dist_51", "tri.th_low", "rejected", [F(100.0, 50.0)], [F(120.0, 50.0, 51)], [-1]))
_t("tri_tie2_last_wins", "tri.tie", "two: the last", [F(100.0, 50.0)], [F(120.0, 50.0, 20), F(130.0, 50.0, 20, at=128)], [1])
_t("tri_tie3_last_wins", "tri.tie", "three: the last", [F(100.0, 50.0)], [F(120.0, 50.0, 20), F(130.0, 50.0, 20, at=64), F(140.0, 50.0, 20, at=128)], [2])
_t("tri_tie3_last_fails_epipolar", "tri.tie", "three, the last off the line: the second",
   [F(100.0, 50.0)], [F(120.0, 50.0, 20), F(130.0, 50.0, 20, at=64), F(140.0, 55.0, 20, at=128)], [1])
_t("tri_tie_then_better", "tri.tie", "a smaller distance first: later larger ones lose", [F(100.0, 50.0)], [F(120.0, 50.0, 19), F(130.0, 50.0, 20, at=128)], [0])
# a query takes the partner, the next query of the node with the same preference takes the other (the hand-over with a tie)
_t("tri_tie_two_queries", "tri.tie", "two queries: the last, then the one before", [F(100.0, 50.0), F(101.0, 50.0, 2, at=200)],
   [F(120.0, 50.0, 20), F(130.0, 50.0, 20, at=128)], [1, 0])


def _bisect_tri(name, decision, sides, scene, lo, hi):
    kw = dict(only_stereo=False, check_orientation=False)
    a, b = bisect(lambda t: outcome("tri", scene(t), kw), lo, hi)
    na = add(name + "_" + sides[0].replace(" ", "_"), "tri", decision, sides[0], scene(a), [0], **kw)
    nb = add(name + "_" + sides[1].replace(" ", "_"), "tri", decision, sides[1], scene(b), [-1], **kw)
    BISECTED[name] = (a, b)
    pair(na, nb)


for _o in (0, 7):  # the epipole on the partner's row, both features mono: skipped when nearer than sqrt(100 sf[oct])
    _bisect_tri("tri_epipole_oct_%d" % _o, "tri.epipole", ("kept", "near the epipole"),
                lambda t, o=_o: tri_scene([F(100.0, 50.0)], [F(300.0, 50.0, 5, oct=o)], epipole=np.array([t, 50.0], f32)), f32(400.0), f32(300.0))
_t("tri_epipole_stereo_1", "tri.epipole", "key-frame 1 stereo: no test", [F(100.0, 50.0, ur=90.0)], [F(300.0, 50.0, 5)], [0], epipole=np.array([300.0, 50.0], f32))
_t("tri_epipole_stereo_2", "tri.epipole", "key-frame 2 stereo: no test", [F(100.0, 50.0)], [F(300.0, 50.0, 5, ur=290.0)], [0], epipole=np.array([300.0, 50.0], f32))
_t("tri_epipole_both_mono", "tri.epipole", "near the epipole", [F(100.0, 50.0)], [F(300.0, 50.0, 5)], [-1], epipole=np.array([300.0, 50.0], f32))
for _o in (0, 7):  # the partner's distance from the line v2 = 50, over the doubles
    _bisect_tri("tri_epipolar_oct_%d" % _o, "tri.epipolar", ("on the line", "off the line"),
                lambda t, o=_o: tri_scene([F(100.0, 50.0)], [F(120.0, float(t), 5, oct=o)]), f64(50.0), f64(62.0))
pair(_t("tri_den_zero", "tri.den", "den == 0", [F(100.0, 50.0)], [F(120.0, 50.0, 5)], [-1], fmat=np.zeros((3, 3))),
     _t("tri_den_one", "tri.den", "den == 1", [F(100.0, 50.0)], [F(120.0, 50.0, 5)], [0]))
# only_stereo: a feature asks / is a partner only when u_right >= 0 (-0.0 is)
for _n, _ur, _ok in (("minus_0", -0.0, 1), ("plus_0", 0.0, 1), ("minus_1", -1.0, 0)):
    _t("tri_only_stereo_kf1_ur_" + _n, "tri.stereo", "stereo" if _ok else "mono", [F(100.0, 50.0, ur=_ur)], [F(120.0, 50.0, 5, ur=100.0)], [0 if _ok else -1], only_stereo=True)
    _t("tri_only_stereo_kf2_ur_" + _n, "tri.stereo", "stereo" if _ok else "mono", [F(100.0, 50.0, ur=90.0)], [F(120.0, 50.0, 5, ur=_ur)], [0 if _ok else -1], only_stereo=True)
    # without only_stereo the flag switches the epipole test off
    _t("tri_epipole_kf2_ur_" + _n, "tri.stereo", "stereo" if _ok else "mono", [F(100.0, 50.0)], [F(300.0, 50.0, 5, ur=_ur)], [0 if _ok else -1], epipole=np.array([300.0, 50.0], f32))
pair("tri_only_stereo_kf1_ur_minus_0", "tri_only_stereo_kf1_ur_minus_1")
pair(_t("tri_kf1_has_map_point", "tri.has_mp", "key-frame 1's has", [F(100.0, 50.0, has_mp=1)], [F(120.0, 50.0, 5)], [-1]),
     _t("tri_no_map_points", "tri.has_mp", "neither has", [F(100.0, 50.0)], [F(120.0, 50.0, 5)], [0]))
_t("tri_kf2_has_map_point", "tri.has_mp", "key-frame 2's has: the other partner", [F(100.0, 50.0)], [F(120.0, 50.0, 5, has_mp=1), F(130.0, 50.0, 30, at=128)], [1])

# ================================================ searchByBoW ===========================================================================
def _b(name, decision, side, fk, ff, want, nn_ratio=0.8, chk=False, **sc):
    return add(name, "bow", decision, side, bow_scene(fk, ff, **sc), want, nn_ratio=nn_ratio, check_orientation=chk)


_K = lambda k=0, at=0, **kw: F(0, 0, k, at=at, has_mp=1, **kw)
_FR = lambda k=0, at=0, **kw: F(0, 0, k, at=at, **kw)
pair(_b("bow_dist_50", "bow.th_low", "accepted", [_K()], [_FR(50)], [0]),
     _b("bow_dist_51", "bow.th_low", "rejected", [_K()], [_FR(51)], [-1]))
for _b1, _b2, _rt, _ok in ((4, 5, 0.8, 0), (3, 5, 0.8, 1), (40, 50, 0.8, 0), (39, 50, 0.8, 1), (3, 5, 0.6, 0), (2, 5, 0.6, 1)):
    _b("bow_ratio_%d_%d_at_%g" % (_b1, _b2, _rt), "bow.ratio", "accepted" if _ok else "rejected", [_K()], [_FR(_b1), _FR(_b2, at=128)], [0 if _ok else -1, -1], nn_ratio=_rt)
pair("bow_ratio_4_5_at_0.8", "bow_ratio_3_5_at_0.8")
pair("bow_ratio_40_50_at_0.8", "bow_ratio_39_50_at_0.8")
pair("bow_ratio_3_5_at_0.6", "bow_ratio_2_5_at_0.6")
_b("bow_single_partner", "bow.ratio", "one partner: the second best is 256", [_K()], [_FR(50)], [0], nn_ratio=0.2)
pair(_b("bow_tie", "bow.tie", "tie: rejected", [_K()], [_FR(20), _FR(20, at=128)], [-1, -1]),
     _b("bow_no_tie", "bow.tie", "19 / 30: accepted", [_K()], [_FR(19), _FR(30, at=128)], [0, -1]))
_b("bow_tie_ratio_off", "bow.tie", "tie with the ratio test off: the first", [_K()], [_FR(20), _FR(20, at=128)], [0, -1], nn_ratio=1.1)
# query 0 (the word itself) sees 20 / 22 and rejects; query 1 (partner 0's own word) then finds partner 0 still free
pair(_b("bow_reject_claims_nothing", "bow.reject_claims_nothing", "the first rejects: the second takes its best", [_K(), _K(20, at=0)], [_FR(20), _FR(22, at=128)], [1, -1]),
     _b("bow_accept_claims", "bow.reject_claims_nothing", "the first accepts: the second is left with the other partner", [_K(), _K(20, at=0)], [_FR(10), _FR(22, at=128)], [0, 1]))
pair(_b("bow_node_shared", "bow.node", "shared", [_K()], [_FR(5)], [0], nodes1={7: [0]}, nodes2={7: [0]}),
     _b("bow_node_not_shared", "bow.node", "not shared", [_K()], [_FR(5)], [-1], nodes1={7: [0]}, nodes2={8: [0]}))
_b("bow_node_lists_interleaved", "bow.node", "ids 3, 7 against 5, 7", [_K(), _K(0, at=0)], [_FR(5), _FR(6, at=128)], [-1, 1], nodes1={3: [0], 7: [1]}, nodes2={5: [0], 7: [1]})
_b("bow_empty_list", "bow.node", "the frame's list of the node is empty", [_K()], [_FR(5)], [-1], nodes1={7: [0]}, nodes2={7: [], 9: [0]})
pair(_b("bow_no_map_point", "bow.has_mp", "no map point", [F(0, 0, 0, has_mp=0)], [_FR(5)], [-1]),
     _b("bow_map_point", "bow.has_mp", "map point", [_K()], [_FR(5)], [0]))

# ================================================ the fuse search ===================================================================
def _u(name, decision, side, feats, qs, want, dist, th=3.0):
    s = proj_scene(feats, qs)
    s["mp_level"] = s["mp_level"].astype(np.int32)
    return add(name, "fuse", decision, side, s, want, dist=dist, th=th)


pair(_u("fuse_dist_50", "fuse.th_low", "accepted", [F(X0, Y0, 50)], [Q(X0, Y0)], [0], [50]),
     _u("fuse_dist_51", "fuse.th_low", "rejected", [F(X0, Y0, 51)], [Q(X0, Y0)], [-1], [51]))
_u("fuse_tie_two_cells", "fuse.th_low", "tie: the first in visiting order (the left column)", [F(300.5, Y0, 20), F(298.5, Y0, 20, at=128)], [Q(299.5, Y0)], [1], [20])
_u("fuse_tie_one_cell", "fuse.th_low", "tie: the lower index", [F(X0, Y0, 20), F(X0 + 1, Y0, 20, at=128)], [Q(X0, Y0)], [0], [20])


# the window of the fuse search binds only below th = 2.45 (above, the chi2 gate is the narrower one): th = 2, a window of exactly 2.0
pair(_u("fuse_x_plus_r", "grid.window_strict", "outside", [F(X0 + 2.0, Y0, 5)], [Q(X0, Y0)], [-1], [256], th=2.0),
     _u("fuse_x_plus_r_float_below", "grid.window_strict", "inside", [F(f64(below(f32(X0 + 2.0))), Y0, 5)], [Q(X0, Y0)], [0], [5], th=2.0))
pair(_u("fuse_y_plus_r", "grid.window_strict", "outside", [F(X0, Y0 + 2.0, 5)], [Q(X0, Y0)], [-1], [256], th=2.0),
     _u("fuse_y_plus_r_float_below", "grid.window_strict", "inside", [F(X0, f64(below(f32(Y0 + 2.0))), 5)], [Q(X0, Y0)], [0], [5], th=2.0))


def _bisect_fuse(name, sides, scene, lo, hi):
    kw = dict(th=3.0)
    res = lambda s: tuple(int(v) for r in run(numpy_ref, "fuse", s, kw)[::2] for v in r)
    a, b = bisect(lambda t: res(scene(t)), f64(lo), f64(hi))
    for x, sd, bi, bd in ((a, sides[0], [0], [5]), (b, sides[1], [-1], [256])):  # inside: the feature, 5 bits off; outside: nothing
        add(name + "_" + sd.replace(" ", "_"), "fuse", "fuse.chi2", sd, scene(x), bi, dist=bd, **kw)
    BISECTED[name] = (a, b)
    pair(name + "_" + sides[0].replace(" ", "_"), name + "_" + sides[1].replace(" ", "_"))


def _fuse1(feat, q):
    s = proj_scene([feat], [q])
    s["mp_level"] = s["mp_level"].astype(np.int32)
    return s


for _o in (0, 3):  # the query's x over the doubles: mono err = dx^2 / sigma2[oct] against 5.99, stereo (dz = 0) against 7.8
    _bisect_fuse("fuse_chi2_mono_oct_%d" % _o, ("inside", "outside"), lambda t, o=_o: _fuse1(F(X0, Y0, 5, oct=o), Q(float(t), Y0, lvl=o)), X0, X0 + 3.0 * 1.2 ** _o)
    _bisect_fuse("fuse_chi2_stereo_oct_%d" % _o, ("inside", "outside"), lambda t, o=_o: _fuse1(F(X0, Y0, 5, oct=o, ur=280.0), Q(float(t), Y0, ur=280.0, lvl=o)), X0, X0 + 3.0 * 1.2 ** _o)
# dx = 2.6: err = 6.76, between the two gates; u_right chooses the gate (dz = 0 - 0)
for _n, _ur, _st in (("minus_1", -1.0, 0), ("minus_0", -0.0, 1), ("plus_0", 0.0, 1)):
    _u("fuse_gate_ur_" + _n, "fuse.chi2", "stereo gate 7.8" if _st else "mono gate 5.99", [F(X0, Y0, 5, ur=_ur)], [Q(X0 + 2.6, Y0, ur=0.0)], [0 if _st else -1], [5 if _st else 256])
pair("fuse_gate_ur_minus_1", "fuse_gate_ur_minus_0")
for _lvl in (0, 7):
    for _o, _ok in ((_lvl - 2, 0), (_lvl - 1, 1), (_lvl, 1), (_lvl + 1, 0)):
        if 0 <= _o <= 7:
            _u("fuse_level_%d_octave_%d" % (_lvl, _o), "fuse.level_band", "inside" if _ok else "outside", [F(X0, Y0, 5, oct=_o)], [Q(X0, Y0, lvl=_lvl)],
               [0 if _ok else -1], [5 if _ok else 256])
pair("fuse_level_0_octave_0", "fuse_level_0_octave_1")
pair("fuse_level_7_octave_5", "fuse_level_7_octave_6")


# ================================================ regime cases ====================================================================
def visiting_order(uv, size):
    """the order getFeaturesInArea visits the gridded features of `uv` in: cell column, cell row, index (cells by std::round)"""
    rnd = lambda v: np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)
    px, py = rnd(uv[:, 0] * f64(f32(64) / f32(size[0]))), rnd(uv[:, 1] * f64(f32(48) / f32(size[1])))
    order = np.lexsort((np.arange(len(uv)), py, px))
    return order[((px >= 0) & (px < 64) & (py >= 0) & (py < 48))[order]]


def _window_distances(n_feat, strict):
    """distance by visiting position.  Not strict: groups of four equal ones falling towards the end, so every query's best are the LAST
    candidates and ties are decided by position.  Strict: 5, 6, 7, .. (at most 90) counted from the last candidate backwards, so the LAST
    candidate (position n_feat - 1) is the best of all, the one before it the second best, ..."""
    p = np.arange(n_feat)
    return np.minimum(5 + (n_feat - 1 - p), 90) if strict else 5 + (n_feat - 1 - p) // 4


def _wide(n_feat, x0, y0):
    ij = [(i, j) for i in range(18) for j in range(17)][:n_feat]
    return np.array([[x0 + 2 * i, y0 + 2 * j] for i, j in ij], f64)


def wide_window(n_feat=300, n_query=6, strict=False):
    """n_feat features of octave 0 in ONE window (th = 5: 20 px), none taken; 6 queries on it that all prefer the same features (distances:
    _window_distances) -> (scene, kw, the features in visiting order).  A query's packed record holds a candidate's position in 8 bits:
    256 candidates are the most that are keyed, the 257th (position 256) is the first that is not.  Strict with 256 / 257 features: the
    best candidate is the one at position 255 / 256, the records hold the last three, and the queries 1 and 2 decide from their records
    in the rounds 2 and 3 (query 3 has lost all three keys and walks again)"""
    uv = _wide(n_feat, 283.0, 184.0)
    order = visiting_order(uv, (W0, H0))
    k = np.zeros(n_feat, int)
    k[order] = _window_distances(n_feat, strict)
    feats = [F(uv[i, 0], uv[i, 1], int(k[i]), at=(37 * i) % 256) for i in range(n_feat)]
    return proj_scene(feats, [Q(X0, Y0) for _ in range(n_query)]), dict(th=5.0, nn_ratio=1.1), order


def wide_window_frame(n_feat=300, n_query=6, strict=False):
    """the same features for the last-frame search: th = 20, 6 points that project to (cx, cy)"""
    uv = _wide(n_feat, 350.0, 236.0)
    order = visiting_order(uv, (W0, H0))
    k = np.zeros(n_feat, int)
    k[order] = _window_distances(n_feat, strict)
    feats = [F(uv[i, 0], uv[i, 1], int(k[i]), at=(37 * i) % 256) for i in range(n_feat)]
    return frame_scene(feats, [_PT] * n_query), dict(th=20.0, mono=False, check_orientation=False), order


# (features, strict): the last keyed size, the first that is not, and well beyond
WIDE_WINDOWS = ((256, True), (257, True), (300, False))


def conflict_chain(NF=40, NP=2500, float_uv=True):
    """tests/test_gpu_match.py's conflict chain with 2 500 map points: feature i is i bits from the word every map point holds, every
    map point has every feature in its window -> query k gets feature k for k < 40, nothing after.  From round 3 on the ~2 460 unsettled
    queries have lost two of their three cached keys: more than the re-walk list holds (2 048 in the 1 024-thread shape)"""
    rng = np.random.default_rng(3)
    uv = np.tile([[300.0, 200.0]], (NF, 1)) + rng.uniform(-3, 3, (NF, 2))
    if float_uv:
        uv = uv.astype(f32).astype(f64)
    feats = [F(uv[i, 0], uv[i, 1], i, at=(11 * i) % 256) for i in range(NF)]
    return proj_scene(feats, [Q(300.0, 200.0, ur=250.0) for _ in range(NP)]), dict(th=3.0, nn_ratio=1.1)


def deep_chain(matcher, n=12, rejecting=None, tie=False):
    """one node, n partners in strict preference order (partner j is 2 + 2 j bits from the word), n queries that all hold the word: query
    m gets partner m; from the fourth on a query has lost all three cached keys.  rejecting (bow): that query sees the partners at
    distances that fail the ratio test (it holds a word 20 bits off: every partner at about 20) and claims nothing.  tie (tri): partners
    2 j and 2 j + 1 are equally far - the LAST of a tie wins, so the queries take 1, 0, 3, 2, ..."""
    if matcher == "bow":
        fk = [_K(0) for _ in range(n)]
        ff = [_FR(2 + 2 * j, at=0) for j in range(n)]
        if rejecting is not None:
            fk[rejecting] = F(0, 0, 10, at=128, has_mp=1)  # 10 bits further from every partner: 22 < 0.9 x 24 fails
        return bow_scene(fk, ff), dict(nn_ratio=1.1 if rejecting is None else 0.9, check_orientation=False)
    f1 = [F(100.0 + j, 50.0) for j in range(n)]
    f2 = [F(120.0 + j, 50.0, 2 + 2 * (j // 2 if tie else j), at=0 if not tie or j % 2 == 0 else 100) for j in range(n)]
    return tri_scene(f1, f2), dict(only_stereo=False, check_orientation=False)


def big_node(matcher, n2=1030, n1=8, winner=1027, best=3, second=6, nn_ratio=1.1):
    """one node of n2 partners (every one 30 + (j % 16) bits off in its own bits; the winner `best` off, the partner two places before it
    `second` off, partner 5 8 off), n1 queries that all hold the word: a partner past position 1 023 of a list cannot be keyed -> (data, kw)"""
    ks = [30 + (j % 16) for j in range(n2)]
    ks[winner], ks[winner - 2], ks[5] = best, second, 8
    if matcher == "bow":
        fk = [_K(0) for _ in range(n1)]
        ff = [_FR(ks[j], at=(29 * j) % 256) for j in range(n2)]
        return bow_scene(fk, ff), dict(nn_ratio=nn_ratio, check_orientation=False)
    f1 = [F(100.0 + j, 50.0) for j in range(n1)]
    f2 = [F(120.0 + (j % 500), 50.0, ks[j], at=(29 * j) % 256) for j in range(n2)]
    return tri_scene(f1, f2), dict(only_stereo=False, check_orientation=False)


# (n2, position of the winner, its distance, distance of the partner two before it, nn_ratio): the first size with a partner that cannot be
# keyed and the winner there, a few more, and the last keyed size.  At 1 025 the winner is 2 bits off and the next 3: searchByBoW's key
# holds the position above bit 12 and the distance above bit 22, so a position of 1 024 put into a key would set the lowest bit of the
# distance - 2 would read as 3, and 3 / 3 fails the ratio test at 0.8 that 2 / 3 passes (a distance of 3 would hide it: the bit is set)
BIG_NODES = ((1030, 1027, 3, 6, 1.1), (1025, 1024, 2, 3, 0.8), (1024, 1023, 3, 6, 1.1))


# ---- the general walk: one more feature whose coordinates are doubles that are no floats, far from every window ---------------------
def with_double_feature(case):
    """-> (data, want) of the case with such a feature appended (it matches nothing: 200 bits off, no window near it).  The kernels choose
    the walk per frame: with it, every feature of the frame is tested as (float)(u - (double)x), not as a packed float record"""
    assert case.matcher in ("proj", "frame", "fuse")
    d = dict(case.data)
    at = (300.123456789, 250.3) if case.size == (WG, HG) else ((700.123456789, 440.3) if case.matcher == "frame" else (600.123456789, 400.3))
    assert f64(f32(at[0])) != at[0]
    d["feat_uv"] = np.concatenate([d["feat_uv"], [at]])
    d["feat_ur"] = np.concatenate([d["feat_ur"], f32([-1.0])])
    d["feat_oct"] = np.concatenate([d["feat_oct"], np.int32([0])])
    d["feat_desc"] = np.concatenate([d["feat_desc"], desc(200, 17)[None]])
    for k in ("feat_taken", "feat_angle"):
        if k in d:
            d[k] = np.concatenate([d[k], np.zeros(1, d[k].dtype)])
    want = case.want if case.matcher == "fuse" else np.concatenate([case.want, np.int32([-1])])
    return d, want


# ---- the local-map cases as 3-D points (gl_search_local_points: gl_project_map_points, then the search) ------------------------------
def as_points3d(case):
    """the queries of a local-map case as map points in front of a camera at the origin, 5 m away: position on the pixel's ray, predicted
    level from max_dist = dist x 1.2 ^ (lvl - 0.5), the normal 0.8 in cosine off the viewing ray (the 4.0 window, as cos = 0.5 in the
    cases).  -> the inputs of project_map_points, or None where the case cannot be said this way: a query outside the image is not in
    view, u_right is the projection's own (bf / z), and a viewing cosine cannot be placed to the bit"""
    d = case.data
    if case.matcher != "proj" or case.decision in ("proj.u_right", "proj.viewcos"):
        return None
    x, y = d["mp_uvr"][:, 0], d["mp_uvr"][:, 1]
    if not ((x >= 0) & (x < d["width"]) & (y >= 0) & (y < d["height"])).all():
        return None
    z = 5.0
    pos = np.stack([(x - f64(f32(CAM.cx))) / f64(f32(CAM.fx)) * z, (y - f64(f32(CAM.cy))) / f64(f32(CAM.fy)) * z, np.full(len(x), z)], 1)
    dist = np.linalg.norm(pos, axis=1)
    v = pos / dist[:, None]
    w = np.cross(v, [0.0, 1.0, 0.0])
    w /= np.linalg.norm(w, axis=1)[:, None]
    return dict(pose_cw=np.array([0, 0, 0, 1, 0, 0, 0], f64), t_wc=np.zeros(3), pos=pos, normal=0.8 * v + 0.6 * w,
                max_dist=(dist * 1.2 ** (d["mp_level"] - 0.5)).astype(f32), min_dist=(0.1 * dist).astype(f32), cand=d["mp_valid"].copy())


def capacity_scenes():
    """every entry point at the largest sizes its GL_REQUIRE states, on synth scenes with dense conflicts: projection 3 072 / 4 096 (both
    overloads, both coordinate kinds), triangulation and BoW 4 096 / 4 096 (crowded nodes), fuse 16 384 -> {name: (matcher, data, kw)}"""
    from gmmloc_amd import synth
    out = {}
    for fuv in (True, False):
        out["proj_float_uv_%d" % fuv] = ("proj", synth.synth_match_frame(3072, 4096, 901 + fuv, dup_frac=0.9, float_uv=fuv), dict(th=3.0, nn_ratio=0.8))
        out["fuse_float_%d" % fuv] = ("fuse", synth.synth_fuse_frame(16384, 4096, 906 + fuv, float_coords=fuv), dict(th=3.0))
    out["frame"] = ("frame", synth.synth_motion_frames(3072, 4096, 903, CAM), dict(th=7.0, mono=False, check_orientation=True))
    tri = synth.synth_tri_search_pair(4096, 4096, 904, CAM, n_nodes=100)
    out["tri"] = ("tri", tri, dict(only_stereo=False, check_orientation=True))
    out["tri_only_stereo_no_orientation"] = ("tri", tri, dict(only_stereo=True, check_orientation=False))
    bow = synth.synth_bow_pair(4096, 4096, 905, CAM, n_nodes=100)
    out["bow"] = ("bow", bow, dict(nn_ratio=0.7, check_orientation=True))
    out["bow_0.9_no_orientation"] = ("bow", bow, dict(nn_ratio=0.9, check_orientation=False))
    return out
