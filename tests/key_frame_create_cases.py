"""Hand-built key-frames on both sides of every decision of the two depth-ordered walks, GMMLoc::createMapPointsFromStereo
(gmmloc_opt.cpp:36-113) and Tracking::createTemporalPoints (tracking.cpp:411-465), in the manner of tests/keyframe_cases.py, whose camera
(CAM5), pose (ID7), planes (PL, FAR_FAIL) and axis_feature they reuse.  Test infrastructure for tests/test_key_frame_create_ref.py (CPU:
the sequential model of tests/key_frame_create_ref.py gives every output a case declares, with the oracle's check and with numpy_ref's)
and tests/test_gpu_key_frame_create.py (the device gives them too).

Every feature lies on the optical axis - features may share a pixel - so its unprojected point is (0, 0, depth) and its u_right is
256 - 64 / depth; what differs between features is the depth, the held state and the candidate list.  th_depth is 1.5f: a "near" entry
has depth 1, a "far" one depth 2.  The check's three answers come from scenes of tests/keyframe_cases.py:
  MAP_ONE  = [PL(2.001)]            candidate [0] at depth 2: accepted, component 0, the point moves        (cma_one_candidate)
                                    ncand = 5 with every entry -1: the fallback moves the point, -1          (cma_all_minus_1)
  MAP_MOVE = [FAR_FAIL, PL(2.002)]  candidate [0] at depth 2: fails, the fallback moves the point, -1        (cma_fallback_degenerate_moves)
                                    candidate [1] at depth 2: accepted, component 1
  MAP_K1   = [FAR_FAIL]             candidate [0]: fails, the fallback fails again, the point is untouched, -1   (cma_fallback_K1)
A case declares EVERY output: the created points in walk order as (feature, component) - from which new_feat, new_assoc, att_feat,
new_ref_kf = att_kf = kf_row, att_mp = mp_base + r, n_new and the r entries of feat_new follow - the -2 slots of feat_new, the eight
stats, the depth of every entry (pts0 is (0, 0, depth)) and which created points the check moved.  PAIRS: two cases whose declared
`stats` differ in exactly the named elements.

The decisions (DECISIONS holds the same list):
  kfc.entry    :39-44   depth > 0 as a float compare                  +0.0, -0.0, 1e-45f, -1, NaN, +inf; a padding slot with positive depth
  kfc.order    :49      ascending (depth, index)                      equal depths; one ulp apart with the higher index nearer; an order that
                                                                      differs from the index order across and inside the compaction
  kfc.held     :55-63   null / observed / without observation         0, 1, 2; 2 accepted and rejected
  kfc.check    :72-95   ncand == 0: FromDepth, no check; a null       ncand 0; accepted; rejected moved / untouched; ncand 5 all -1
                        answer is a `continue`
  kfc.break    :109     check_depth && depth > th_depth &&            num_points 100 / 101; depth == th_depth / one ulp above; check_depth 0; the
                        num_points > 100, after a counted entry       triggering entry created / held; a rejected entry where the test would
                                                                      first hold; 101 entries with an early rejected one; held 2 behind the break
  tmp.break    tracking.cpp:462   depth > th_depth && num_pts > 100   the same break cases, always armed
  tmp.outlier  orb_matcher.cpp:432  the slot's is_outlier_ survives   last_outlier 0 / 1 on a created slot
  tmp.held     tracking.cpp:437-453  a held key-point stays           held 1 keeps its row's bytes; held 2 walked is replaced, behind the break not"""
import numpy as np

from tests.keyframe_cases import CAM5, FAR_FAIL, ID7, PL, above, axis_feature, mk_map

f32, f64 = np.float32, np.float64
TH = f32(1.5)
NEAR, FAR = f32(1.0), f32(2.0)
MP_BASE, KF_ROW = 1000, 7
MAP_ONE, MAP_MOVE, MAP_K1 = [PL(2.001)], [FAR_FAIL, PL(2.002)], [FAR_FAIL]

DECISIONS = {"kfc.entry": "gmmloc_opt.cpp:39-44", "kfc.order": "gmmloc_opt.cpp:49", "kfc.held": "gmmloc_opt.cpp:55-63", "kfc.check": "gmmloc_opt.cpp:72-95",
             "kfc.break": "gmmloc_opt.cpp:109", "tmp.break": "tracking.cpp:462", "tmp.outlier": "orb_matcher.cpp:432", "tmp.held": "tracking.cpp:437-453"}


def feat(depth, held=0, cand=(), ncand=None, oct=0, outlier=0):
    return dict(depth=f32(depth), held=held, cand=tuple(cand), ncand=len(cand) if ncand is None else ncand, oct=oct, outlier=outlier)


def frame(feats, k=5):
    """the arrays of one key-frame from its features: all on the optical axis, u_right from the depth where that is a positive number"""
    NF = len(feats)
    _, u1 = axis_feature(1.0)
    fr = dict(pose=ID7.copy(), feat_uv=np.tile(u1[:2], (NF, 1)).astype(f64), feat_ur=np.zeros(NF, f32), feat_depth=np.array([f["depth"] for f in feats], f32),
              feat_oct=np.array([f["oct"] for f in feats], np.int32), cand=-np.ones((NF, k), np.int32), ncand=np.array([f["ncand"] for f in feats], np.int32),
              held=np.array([f["held"] for f in feats], np.uint8), last_outlier=np.array([f["outlier"] for f in feats], np.uint8))
    for i, f in enumerate(feats):
        d = float(f["depth"])
        fr["feat_ur"][i] = f32(256.0 - 64.0 / d) if np.isfinite(d) and d > 1e-3 else f32(-1.0)
        fr["cand"][i, :len(f["cand"])] = f["cand"]
    # descriptors that name their slot, so that a copied row is recognised
    fr["feat_desc"] = ((np.arange(NF)[:, None] * 7 + np.arange(32)[None] * 3 + 1) % 251).astype(np.uint8)
    return fr


class Case:
    def __init__(self, name, call, decision, side, comps, feats, want, k=5, check_depth=1, th=TH):
        assert decision in DECISIONS, decision
        self.name, self.call, self.decision, self.side, self.want = name, call, decision, side, want
        self.mean, self.cov = mk_map(comps)
        self.cam, self.k, self.check_depth, self.th, self.feats = CAM5, k, check_depth, f32(th), feats
        self.fr = frame(feats, k)
        self.NF = len(feats)

    def __repr__(self):
        return self.name


CASES, PAIRS = {}, []


def stats(entries, walked, n_new, rejected, num, broke):
    return np.array([entries, walked, n_new, rejected, num, broke, 0, 0], np.int32)


def S(name, decision, side, comps, feats, new, st, null=(), moved=(), **kw):
    """a createMapPointsFromStereo case.  new: [(feature, component)] in walk order; null: the slots left at -2; moved: the created
    features whose point the check moved (every other created point is its pts0, bit for bit)"""
    assert name not in CASES, name
    NF, n = len(feats), len(new)
    feat_new = -np.ones(NF, np.int32)
    for i in null:
        feat_new[i] = -2
    for r, (i, _) in enumerate(new):
        feat_new[i] = r
    i32 = lambda a: np.array(a, np.int32).reshape(-1)
    want = dict(new_feat=i32([i for i, _ in new]), new_assoc=i32([c for _, c in new]), new_ref_kf=i32([KF_ROW] * n), att_mp=i32([MP_BASE + r for r in range(n)]),
                att_kf=i32([KF_ROW] * n), att_feat=i32([i for i, _ in new]), n_new=n, feat_new=feat_new, stats=st, moved=tuple(moved))
    assert st[2] == n
    CASES[name] = Case(name, "stereo", decision, side, comps, feats, want, **kw)
    return name


def pair(a, b, elems):
    PAIRS.append((a, b, tuple(elems)))


ENTRIES, WALKED, N_NEW, REJECTED, NUM, BROKE = range(6)

# ---- kfc.entry
_DEPTHS = [f32(0.0), f32(-0.0), f32(1e-45), f32(-1.0), f32(np.nan), f32(np.inf), f32(1.0)]
S("entry_depths", "kfc.entry", "+0 -0 -1 NaN out; 1e-45f, 1, +inf in, in that order", MAP_K1, [feat(d) for d in _DEPTHS], [(2, -1), (6, -1), (5, -1)],
  stats(3, 3, 3, 0, 3, 0))
S("entry_padding", "kfc.entry", "a padding slot (octave -1, 8) with positive depth: never an entry", MAP_K1, [feat(1.0, oct=-1), feat(1.0), feat(0.5, oct=8)], [(1, -1)],
  stats(1, 1, 1, 0, 1, 0))
S("entry_octave_7", "kfc.entry", "octaves 0 and 7: entries", MAP_K1, [feat(1.0, oct=7), feat(1.0), feat(0.5, oct=0)], [(2, -1), (0, -1), (1, -1)], stats(3, 3, 3, 0, 3, 0))
pair("entry_padding", "entry_octave_7", (ENTRIES, WALKED, N_NEW, NUM))

# ---- kfc.order
S("order_equal_depths", "kfc.order", "bit-equal depths: by index", MAP_K1, [feat(1.0)] * 4, [(0, -1), (1, -1), (2, -1), (3, -1)], stats(4, 4, 4, 0, 4, 0))
S("order_one_ulp", "kfc.order", "one ulp apart, the higher index nearer: it comes first", MAP_K1, [feat(above(f32(1.0))), feat(1.0)], [(1, -1), (0, -1)], stats(2, 2, 2, 0, 2, 0))
# sorted: 4 (0.25), 1 (0.5, held: counted, not created), 3 (0.75), 2 (1.0), 0 (1.25): the walk order is no index order, and the created
# points skip feature 1
S("order_across_and_inside", "kfc.order", "neither the walk nor the compacted list is in index order", MAP_K1,
  [feat(1.25), feat(0.5, held=1), feat(1.0), feat(0.75), feat(0.25)], [(4, -1), (3, -1), (2, -1), (0, -1)], stats(5, 5, 4, 0, 5, 0))

# ---- kfc.held / kfc.check (depth 2 entries, check_depth on: num_points stays far below 100)
S("held_0", "kfc.held", "null: a point is created", MAP_K1, [feat(2.0, held=0)], [(0, -1)], stats(1, 1, 1, 0, 1, 0))
S("held_1", "kfc.held", "a point with observations: counted, nothing created", MAP_K1, [feat(2.0, held=1)], [], stats(1, 1, 0, 0, 1, 0))
S("held_2", "kfc.held", "a point without observation: replaced", MAP_K1, [feat(2.0, held=2)], [(0, -1)], stats(1, 1, 1, 0, 1, 0))
pair("held_0", "held_1", (N_NEW,))
S("held_1_with_candidates", "kfc.held", "held: the check is not run (it would reject)", MAP_K1, [feat(2.0, held=1, cand=[0])], [], stats(1, 1, 0, 0, 1, 0))
S("held_2_accepted", "kfc.held", "without observation, accepted: the slot takes the new point", MAP_MOVE, [feat(2.0, held=2, cand=[1])], [(0, 1)], stats(1, 1, 1, 0, 1, 0),
  moved=(0,))
S("held_2_rejected", "kfc.held", "without observation, rejected: set to null and left so", MAP_MOVE, [feat(2.0, held=2, cand=[0])], [], stats(1, 1, 0, 1, 0, 0), null=(0,))
S("held_0_rejected", "kfc.held", "null, rejected: untouched", MAP_MOVE, [feat(2.0, held=0, cand=[0])], [], stats(1, 1, 0, 1, 0, 0))
pair("held_2_accepted", "held_2_rejected", (N_NEW, REJECTED, NUM))
S("check_ncand_0", "kfc.check", "ncand 0: FromDepth without a check", MAP_ONE, [feat(2.0)], [(0, -1)], stats(1, 1, 1, 0, 1, 0))
S("check_accepted", "kfc.check", "a candidate accepted: FromDepthGMM, the point as the check left it", MAP_ONE, [feat(2.0, cand=[0])], [(0, 0)], stats(1, 1, 1, 0, 1, 0),
  moved=(0,))
S("check_rejected_moved", "kfc.check", "rejected, the fallback moved the point: no point", MAP_MOVE, [feat(2.0, cand=[0])], [], stats(1, 1, 0, 1, 0, 0))
S("check_rejected_untouched", "kfc.check", "rejected, the point untouched: no point", MAP_K1, [feat(2.0, cand=[0])], [], stats(1, 1, 0, 1, 0, 0))
S("check_all_minus_1", "kfc.check", "ncand 5, every entry -1: the list is not empty, the check rejects", MAP_ONE, [feat(2.0, ncand=5)], [], stats(1, 1, 0, 1, 0, 0))
pair("check_ncand_0", "check_all_minus_1", (N_NEW, REJECTED, NUM))
pair("check_accepted", "check_rejected_moved", (N_NEW, REJECTED, NUM))
# all of it in one key-frame, k = 8: walk order 5 (1.0), then the depth-2 entries by index
S("check_mixed_frame", "kfc.check", "every answer in one key-frame", MAP_MOVE,
  [feat(2.0, cand=[0]), feat(2.0, cand=[1]), feat(2.0), feat(2.0, held=2, cand=[0, 1]), feat(2.0, held=1, cand=[0]), feat(1.0, held=2, ncand=3), feat(2.0, held=2, cand=[0])],
  [(1, 1), (2, -1), (3, 1)], stats(7, 7, 3, 3, 4, 0), null=(5, 6), moved=(1, 3), k=8)


# ---- kfc.break: near entries first (depth 1 < th_depth), then far ones (depth 2 > th_depth); all without candidates unless said
def _walk(n_near, far, near=None):
    return [feat(NEAR) if near is None else near(i) for i in range(n_near)] + list(far)


def _all(n):
    return [(i, -1) for i in range(n)]


S("break_num_100", "kfc.break", "num_points 100 on a far entry: no break (strict)", MAP_K1, _walk(99, [feat(FAR)]), _all(100), stats(100, 100, 100, 0, 100, 0))
S("break_num_101", "kfc.break", "num_points 101 on a far entry: break, the entry itself created", MAP_K1, _walk(100, [feat(FAR), feat(FAR)]), _all(101),
  stats(102, 101, 101, 0, 101, 1))
S("break_far_from_the_start", "kfc.break", "far entries only: the 101st breaks", MAP_K1, _walk(0, [feat(FAR)] * 103), _all(101), stats(103, 101, 101, 0, 101, 1))
S("break_depth_at_th", "kfc.break", "depth == th_depth at 101: no break (strict); the next far entry breaks", MAP_K1, _walk(100, [feat(TH), feat(FAR), feat(FAR)]), _all(102),
  stats(103, 102, 102, 0, 102, 1))
S("break_depth_above_th", "kfc.break", "depth one ulp above th_depth at 101: break", MAP_K1, _walk(100, [feat(above(TH)), feat(FAR), feat(FAR)]), _all(101),
  stats(103, 101, 101, 0, 101, 1))
pair("break_depth_at_th", "break_depth_above_th", (WALKED, N_NEW, NUM))
S("break_check_depth_0", "kfc.break", "check_depth 0 (the first key-frame): no break", MAP_K1, _walk(100, [feat(FAR), feat(FAR)]), _all(102), stats(102, 102, 102, 0, 102, 0),
  check_depth=0)
pair("break_num_101", "break_check_depth_0", (WALKED, N_NEW, NUM, BROKE))
S("break_on_a_held_entry", "kfc.break", "the triggering entry held: counted, the break holds", MAP_K1, _walk(100, [feat(FAR, held=1), feat(FAR)]), _all(100),
  stats(102, 101, 100, 0, 101, 1))
# the 101st entry is far and rejected: `continue` skips the test with num_points 100; the 102nd is counted (101) and breaks; the 103rd is not walked
S("break_rejected_at_the_position", "kfc.break", "a rejected entry where the test would first hold: the next counted one breaks", MAP_K1,
  _walk(100, [feat(FAR, cand=[0]), feat(FAR), feat(FAR)]), _all(100) + [(101, -1)], stats(103, 102, 101, 1, 101, 1))
S("break_accepted_at_the_position", "kfc.break", "the same entry without candidates: it breaks itself", MAP_K1, _walk(100, [feat(FAR), feat(FAR), feat(FAR)]), _all(101),
  stats(103, 101, 101, 0, 101, 1))
pair("break_rejected_at_the_position", "break_accepted_at_the_position", (WALKED, REJECTED))
S("break_101_entries_one_rejected", "kfc.break", "101 entries, an early one rejected: num_points 100 at the 101st, no break", MAP_K1,
  _walk(100, [feat(FAR)], near=lambda i: feat(NEAR, cand=[0]) if i == 3 else feat(NEAR)), [(i, -1) for i in range(101) if i != 3], stats(101, 101, 100, 1, 100, 0))
S("break_101_entries_none_rejected", "kfc.break", "101 entries: break at the 101st", MAP_K1, _walk(100, [feat(FAR)]), _all(101), stats(101, 101, 101, 0, 101, 1))
pair("break_101_entries_one_rejected", "break_101_entries_none_rejected", (N_NEW, REJECTED, NUM, BROKE))
S("break_held_2_behind", "kfc.break", "a point without observation just behind the break: left alone", MAP_K1, _walk(100, [feat(FAR), feat(FAR, held=2)]), _all(101),
  stats(102, 101, 101, 0, 101, 1))
S("break_held_2_walked", "kfc.break", "the same slot walked (check_depth 0): replaced", MAP_K1, _walk(100, [feat(FAR), feat(FAR, held=2)]), _all(102),
  stats(102, 102, 102, 0, 102, 0), check_depth=0)


# ---- createTemporalPoints ------------------------------------------------------------------------------------------------------------
def last_rows(NF):
    """the chain's last-frame arrays as the host wrote them: values no walk produces, so that an untouched row is recognised"""
    return dict(last_pt=np.arange(NF * 3, dtype=f64).reshape(NF, 3) + 0.125, last_observed=np.full(NF, 1, np.uint8), last_valid=np.full(NF, 3, np.uint8),
                last_desc=np.full((NF, 32), 0xA5, np.uint8))


def Tm(name, decision, side, feats, created, st, invalid=(), **kw):
    """a createTemporalPoints case.  created: the slots that get a temporal point; invalid: those of them left unmatchable (last_valid 0)"""
    assert name not in CASES, name
    NF = len(feats)
    flag = np.zeros(NF, np.uint8)
    flag[list(created)] = 1
    valid = np.full(NF, 3, np.uint8)
    for i in created:
        valid[i] = 0 if i in invalid else 1
    want = dict(temp_flag=flag, n_temp=len(created), stats=st, last_valid=valid, created=tuple(created))
    assert st[2] == len(created)
    CASES[name] = Case(name, "temporal", decision, side, MAP_K1, feats, want, **kw)
    return name


Tm("tmp_num_100", "tmp.break", "num_pts 100 on a far entry: no break", _walk(99, [feat(FAR)]), range(100), stats(100, 100, 100, 0, 100, 0))
Tm("tmp_num_101", "tmp.break", "num_pts 101 on a far entry: break", _walk(100, [feat(FAR), feat(FAR)]), range(101), stats(102, 101, 101, 0, 101, 1))
Tm("tmp_depth_at_th", "tmp.break", "depth == th_depth at 101: no break; the next far entry breaks", _walk(100, [feat(TH), feat(FAR), feat(FAR)]), range(102),
   stats(103, 102, 102, 0, 102, 1))
Tm("tmp_depth_above_th", "tmp.break", "depth one ulp above th_depth at 101: break", _walk(100, [feat(above(TH)), feat(FAR), feat(FAR)]), range(101),
   stats(103, 101, 101, 0, 101, 1))
pair("tmp_depth_at_th", "tmp_depth_above_th", (WALKED, N_NEW, NUM))
Tm("tmp_candidates_ignored", "tmp.break", "no check: an entry the key-frame walk rejects is created and counted", _walk(100, [feat(FAR, cand=[0]), feat(FAR), feat(FAR)]),
   range(101), stats(103, 101, 101, 0, 101, 1))
Tm("tmp_on_a_held_entry", "tmp.break", "the triggering entry held: counted, the break holds", _walk(100, [feat(FAR, held=1), feat(FAR)]), range(100),
   stats(102, 101, 100, 0, 101, 1))
Tm("tmp_outlier_0_1", "tmp.outlier", "last_outlier 0 / 1 on a created slot: matchable / not", [feat(1.0, outlier=0), feat(1.0, outlier=1), feat(1.0, held=2, outlier=1)],
   (0, 1, 2), stats(3, 3, 3, 0, 3, 0), invalid=(1, 2))
Tm("tmp_outlier_none", "tmp.outlier", "the same slots with last_outlier 0: all matchable", [feat(1.0), feat(1.0), feat(1.0, held=2)], (0, 1, 2), stats(3, 3, 3, 0, 3, 0))
Tm("tmp_held", "tmp.held", "held 1 keeps its row; held 2 is replaced; no depth, padding: untouched",
   [feat(1.0, held=1, outlier=1), feat(0.5, held=2), feat(-1.0), feat(1.0, oct=-1), feat(0.75)], (1, 4), stats(3, 3, 2, 0, 3, 0))
Tm("tmp_held_2_behind", "tmp.held", "a point without observation behind the break keeps its row", _walk(100, [feat(FAR), feat(FAR, held=2)]), range(101),
   stats(102, 101, 101, 0, 101, 1))
Tm("tmp_entry_depths", "tmp.break", "the entry test and the order of the key-frame walk", [feat(d) for d in _DEPTHS], (2, 5, 6), stats(3, 3, 3, 0, 3, 0))

STEREO = sorted(n for n, c in CASES.items() if c.call == "stereo")
TEMPORAL = sorted(n for n, c in CASES.items() if c.call == "temporal")
