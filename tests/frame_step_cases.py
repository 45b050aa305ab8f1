"""Hand-built cases for gl_track_frame_end, gl_map_note_replaced and gl_track_frame_next, with DECLARED outputs: one case on each
side of every decision of include/gmmloc_hip.h's rule tables.  tests/test_frame_step_cases.py (CPU) holds the sequential model and the
vectorised restatement to them, tests/test_gpu_frame_step.py the device.  Test infrastructure; nothing in the product imports it."""
import numpy as np

F32 = np.float32
S, M = 10.0, -1.0  # a stereo observation (a right coordinate), a monocular one
NAN = float("nan")


def build_map(points, NKF, NFK, seed=5):
    """points: per row (valid, [(key-frame, slot, S | M), ...]) -> (m, ba): the CSR in the order given, kf_mp from it, kf_uvr[.., 2] = the
    observation's right coordinate (-1 elsewhere), positions and key-frame poses drawn from `seed`"""
    rng = np.random.default_rng(seed)
    NMP = len(points)
    kf_mp = -np.ones((NKF, NFK), np.int32)
    kf_uvr = np.concatenate([rng.uniform(0, 400, (NKF, NFK, 2)), -np.ones((NKF, NFK, 1))], 2)
    ptr, okf, ofeat = [0], [], []
    for p, (_, obs) in enumerate(points):
        for k, f, r in obs:
            assert kf_mp[k, f] == -1, (p, k, f)
            kf_mp[k, f], kf_uvr[k, f, 2] = p, r
            okf.append(k)
            ofeat.append(f)
        ptr.append(len(okf))
    q = rng.standard_normal((NKF, 4))
    m = dict(mp_valid=np.array([v for v, _ in points], np.uint8), obs_ptr=np.array(ptr, np.int32), obs_kf=np.array(okf, np.int32),
             kf_valid=np.ones(NKF, np.uint8), kf_mp=kf_mp, mp_pos=rng.uniform(-4, 4, (NMP, 3)),
             mp_desc=rng.integers(0, 256, (NMP, 32), dtype=np.uint8))
    ba = dict(kf_pose=np.concatenate([q / np.linalg.norm(q, axis=1)[:, None], rng.uniform(-5, 5, (NKF, 3))], 1), kf_uvr=kf_uvr,
              kf_oct=np.zeros((NKF, NFK), np.int32), obs_feat=np.array(ofeat, np.int32), kf_first=0)
    return m, ba


# ---- the small map: 12 points, 3 key-frames of 8 slots.  Weighted counts: p0 2 (one stereo observation), p1 3 (stereo + mono), p2 4 but
# INVALID, p3 none, p4 1 (mono), p5 .. p10 4 or 3, p11 2.
SMALL = [
    (1, [(0, 0, S)]),
    (1, [(0, 1, S), (1, 1, M)]),
    (0, [(0, 2, S), (1, 2, S)]),
    (1, []),
    (1, [(0, 3, M)]),
    (1, [(0, 4, S), (1, 4, S)]),
    (1, [(1, 5, S), (2, 5, S)]),
    (1, [(2, 6, S), (1, 6, M)]),
    (1, [(1, 7, S), (2, 7, S)]),
    (1, [(2, 0, S), (1, 0, S)]),
    (1, [(2, 1, S), (1, 3, S)]),
    (1, [(2, 2, S)]),
]
NKF, NFK, NMP = 3, 8, 12


def small_map():
    return build_map(SMALL, NKF, NFK)


# KeyFrame::countMapPoints of key-frame 0 (slots: p0 p1 p2 p4 p5 null null null): (num_kfs, ref_kf) -> num_ref_matches
COUNT = {(1, 0): 3, (2, 0): 3, (3, 0): 2,  # threshold 2: p0 p1 p5; threshold 3: p1 p5 (p2 is invalid, p4 weighs 1)
         (3, -1): 0, (3, NKF): 0, (1, 2): 6, (3, 2): 5}  # key-frame 2: p9 p10 p11 p6 p7 p8; p11 weighs 2

# ---- gl_track_frame_end: one frame's arrays; NPcap = 4, n_local_mp = 3, NL = 8, th_depth = 4
TH_DEPTH = 4.0
BELOW, ABOVE = float(np.nextafter(F32(4), F32(0))), float(np.nextafter(F32(4), F32(8)))
LOCAL_MP, N_LOCAL_MP = [5, 6, 7, 9], 3
LAST_OBSERVED = [1, 1, 1, 1, 1, 0, 0, 1]
#        feat_mp match_last match_local outlier depth    held_mp  what the slot shows
END = [
    (0, 0, -1, 0, 1.0, 0),        # a point from the last frame, an inlier in the depth range
    (1, 1, 0, 0, 1.0, 5),         # match_local against feat_mp: the local point wins
    (-1, -1, 2, 0, BELOW, 7),     # match_local at n_local_mp - 1; depth one ulp below th_depth: counted
    (8, 2, 3, 0, 4.0, 8),         # match_local at n_local_mp: feat_mp; depth == th_depth: out
    (9, 3, 4, 0, ABOVE, 9),       # match_local at NPcap: feat_mp; depth one ulp above: out
    (0, 4, -1, 1, 2.0, -1),       # an outlier on an observed point: null, counted in num_total only
    (-1, 5, -1, 1, 2.0, -1),      # an outlier on a temporal point: null, the flag stays 1
    (-1, 6, -1, 0, 2.0, -1),      # a temporal point, no outlier: cleared, no inlier
    (-1, -1, -1, 0, 0.0, -1),     # nothing held; depth 0: out
    (1, 7, -1, 0, -0.0, 1),       # depth -0.0: out
    (5, 0, -1, 0, NAN, 5),        # depth NaN: out (a point held twice is held twice)
    (3, 1, -1, 0, 1.0, -1),       # a row without observations: no inlier, cleared
    (4, 2, -1, 0, -1.0, 4),       # one monocular observation is an observation
    (2, 3, -1, 0, 1.5, 2),        # the tail does not ask for validity (the chain has un-held what it found invalid)
]
END_STAT = dict(num_match_inliers=9, num_map=4, num_total=8, ratio_map=0.5)  # total: slots 0 1 2 5 6 7 11 13; map: 0 1 2 13
END_MODES = [0, 2, 1, 0]    # frame 1 is lost, frame 2 went through the key-frame, frame 3 has no depth at all
END_REF_KF = [0, 0, -1, 0]
END_RULE = dict(num_kfs=3, frame_idx=100, kf_frame_idx=90, fps=20.0, is_idle=0, n_queue=0)
#           res nmi map total ref verdict
END_STATS = [[1, 9, 4, 8, 2, 0, 0, 0], [0, 10, 0, 0, 0, 0, 0, 0], [0, 9, 4, 8, 0, 0, 0, 0], [1, 9, 0, 0, 2, 0, 0, 0]]
END_RATIO = [0.5, None, 0.5, 0.0]  # (None: not written)


def end_arrays():
    """-> the arguments of frame_end for the B = 4 frames of END_MODES"""
    col = lambda j, dt: np.array([[r[j] for r in END]] * 4, dt)
    a = dict(feat_mp=col(0, np.int32), match_last=col(1, np.int32), match_local=col(2, np.int32), outlier=col(3, np.uint8),
             local_mp=np.array([LOCAL_MP] * 4, np.int32), n_local_mp=np.full(4, N_LOCAL_MP, np.int32),
             counts2=np.array([[0, 0, 0, mode] for mode in END_MODES], np.int32), ref_kf=np.array(END_REF_KF, np.int32),
             last_observed=np.array([LAST_OBSERVED] * 4, np.uint8), feat_depth=col(4, F32))
    a["feat_depth"][3] = [0.0, -0.0, NAN, -1.0, 4.0, ABOVE, 9.0] * 2
    return a


END_HELD_MP = [r[5] for r in END]

# ---- needNewKeyFrame at its thresholds: the rule map - point p < 304 is seen by key-frame 1 (stereo) and 2 (mono): weight 3; p < 80
# also by key-frame 0 (stereo): 5, and counted there; rows 304 .. 307 by key-frame 0 alone (stereo, weight 2): counted at a threshold of 2
RULE_ROWS, RULE_REF, RULE_NF = 304, 80, 400


def rule_map():
    pts = [(1, ([(0, p, S)] if p < RULE_REF else []) + [(1, p, S), (2, p, M)]) for p in range(RULE_ROWS)]
    pts += [(1, [(0, RULE_REF + j, S)]) for j in range(4)]
    return build_map(pts, 3, RULE_ROWS, seed=6)


def rule_frame(nmi, num_map, num_total):
    """a frame of RULE_NF features: the first nmi hold their own row; depth inside the range for the first num_map of them and for the
    last num_total - num_map features, which hold nothing"""
    assert num_map <= nmi <= RULE_ROWS and nmi + (num_total - num_map) <= RULE_NF
    feat_mp = np.where(np.arange(RULE_NF) < nmi, np.arange(RULE_NF), -1).astype(np.int32)
    depth = np.zeros(RULE_NF, F32)
    depth[:num_map] = 1.0
    depth[RULE_NF - (num_total - num_map):] = 1.0
    none = -np.ones(RULE_NF, np.int32)
    return dict(feat_mp=feat_mp[None], match_last=none[None], match_local=none[None], outlier=np.zeros((1, RULE_NF), np.uint8),
                local_mp=-np.ones((1, 4), np.int32), n_local_mp=np.zeros(1, np.int32), counts2=np.zeros((1, 4), np.int32),
                ref_kf=np.zeros(1, np.int32), last_observed=None, feat_depth=depth[None])


_BASE = dict(num_kfs=3, frame_idx=100, kf_frame_idx=90, fps=20.0, is_idle=0, n_queue=0)
NEED, INTERRUPT = 1, 2
# name: (rule overrides, nmi, num_map, num_total, num_ref_matches, verdict).  ratio_map = num_map / num_total; 3/10, 1/5 and 7/20 round
# to 0.3f, 0.2f and 0.35f exactly; 80 * 0.25f = 20, 80 * 0.75f = 60, 80 * 0.4f = 32 and 84 * 0.75f = 63 are exact, 84 * 0.4f = 33.6
RULES = {
    "quiet": ({}, 100, 10, 10, 80, 0),
    "c1a_at": (dict(frame_idx=110), 59, 10, 10, 80, INTERRUPT | NEED),
    "c1a_one_before": (dict(frame_idx=109), 59, 10, 10, 80, 0),
    "idle": (dict(frame_idx=109, is_idle=1), 59, 10, 10, 80, NEED),
    "busy_queue_2": (dict(frame_idx=110, n_queue=2), 59, 10, 10, 80, INTERRUPT | NEED),
    "busy_queue_3": (dict(frame_idx=110, n_queue=3), 59, 10, 10, 80, INTERRUPT),
    "idle_queue_3": (dict(is_idle=1, n_queue=3), 59, 10, 10, 80, NEED),
    "c1b_inliers_at": ({}, 20, 10, 10, 80, 0),
    "c1b_inliers_below": ({}, 19, 10, 10, 80, INTERRUPT | NEED),
    "c1b_ratio_at": ({}, 59, 3, 10, 80, 0),
    "c1b_ratio_below": ({}, 59, 29, 100, 80, INTERRUPT | NEED),
    "c2_ref_at_kfs3": (dict(is_idle=1), 60, 10, 10, 80, 0),
    "c2_ref_below_kfs3": (dict(is_idle=1), 59, 10, 10, 80, NEED),
    "c2_ref_at_kfs2": (dict(is_idle=1, num_kfs=2), 63, 10, 10, 84, 0),
    "c2_ref_below_kfs2": (dict(is_idle=1, num_kfs=2), 62, 10, 10, 84, NEED),
    "c2_ref_at_kfs1": (dict(is_idle=1, num_kfs=1), 34, 10, 10, 84, 0),
    "c2_ref_below_kfs1": (dict(is_idle=1, num_kfs=1), 33, 10, 10, 84, NEED),
    "c2_map_at_300": (dict(is_idle=1), 300, 7, 20, 80, 0),
    "c2_map_below_300": (dict(is_idle=1), 300, 6, 20, 80, NEED),
    "c2_map_301_same_ratio": (dict(is_idle=1), 301, 6, 20, 80, 0),
    "c2_map_at_301": (dict(is_idle=1), 301, 1, 5, 80, 0),
    "c2_map_below_301": (dict(is_idle=1), 301, 19, 100, 80, NEED),
    "inliers_15": (dict(is_idle=1), 15, 10, 10, 80, 0),
    "inliers_16": (dict(is_idle=1), 16, 10, 10, 80, NEED),
}


def rule_of(name):
    return dict(_BASE, **RULES[name][0])


# ---- gl_map_note_replaced: NMPcap = 14 rows, the steps in order
NMPCAP = 14
REPLACE = {
    "none": ([], {}),
    "one": ([(5, 6)], {5: 6}),
    "chain": ([(5, 6), (6, 7)], {5: 6, 6: 7}),
    "self": ([(8, 8)], {}),
    "repeated": ([(9, 10), (9, 11)], {9: 11}),
    "self_after": ([(9, 10), (9, 9)], {9: 10}),  # (the step that changes nothing does not shadow the one before it)
    "outside": ([(NMPCAP, 0), (0, -1), (-1, 3), (0, NMPCAP), (2 ** 31 - 1, 1)], {}),
    "all": ([(5, 6), (6, 7), (8, 8), (9, 10), (9, 11), (NMPCAP, 0), (0, -1), (-1, 3), (11, 8)], {5: 6, 6: 7, 9: 11, 11: 8}),
}


def replaced_array(name):
    rep = -np.ones(NMPCAP, np.int32)
    for s, t in REPLACE[name][1].items():
        rep[s] = t
    return rep


# ---- gl_track_frame_next on the small map AFTER the steps of REPLACE['all'] and a cull: p5, p6, p9 and p11 are invalid and empty
AFTER = [(0, []) if p in (5, 6, 9, 11) else spec for p, spec in enumerate(SMALL)]
AFTER[8] = (1, SMALL[8][1] + [(0, 7, S)])  # (the target gained an observation)


def after_map():
    return build_map(AFTER, NKF, NFK)


NEXT_HELD = [0, 5, 6, 9, 3, -1, 1, 4, 8, 7]
NEXT_FEAT_NEW, NEXT_MP_BASE = [-1, -1, -1, -1, -1, 0, -2, 1, -1, -1], 10
#            0: kept   1: A -> B (invalid, empty: held 2)   2: B -> C   3: 9 -> 11, itself replaced and invalid: ONE step
#            4: a row without observations   5: a new row, not replaced   6: -2   7: a new row, replaced   8, 9: kept
NEXT_OUT = dict(held_mp=[0, 6, 7, 11, 3, 10, -1, 8, 8, 7], held=[1, 2, 1, 2, 2, 1, 0, 1, 1, 1])
NEXT_OUT_2 = dict(held_mp=[0, 7, 7, 8, 3, 10, -1, 8, 8, 7], held=[1, 1, 1, 1, 2, 1, 0, 1, 1, 1])  # the next frame: B -> C, 11 -> 8
NEXT_PLAIN = dict(held_mp=NEXT_HELD, held=[1, 2, 2, 2, 2, 0, 1, 1, 1, 1])  # without feat_new and mp_replaced
# createTemporalPoints on NEXT_OUT's frame (no key-frame): what frame t + 1 finds as last_mp.  1: the invalid row B becomes a temporal
# point   3: invalid too, but without depth it is not walked: the row stays   4: a valid row without observations: temporal   6: no
# point: temporal   7: depth NaN, not walked   the held == 1 slots keep their rows
NEXT_DEPTH = [1.0, 2.0, 1.5, 0.0, 3.0, 1.0, 2.5, NAN, 1.0, 5.0]
NEXT_TEMPORAL = dict(temp_flag=[0, 1, 0, 0, 1, 0, 1, 0, 0, 0], last_mp=[0, -1, 7, 11, -1, 10, -1, 8, 8, 7])
# malformed rows: outside [-1, NMP) in held_mp (kept, no row), a feat_new beyond the table (nothing), a replacement outside (nothing)
BAD_HELD = [NMP, -2, 2 ** 31 - 1, -2 ** 31, 0, 1]
BAD_FEAT_NEW, BAD_MP_BASE = [-1, -1, -1, -1, 5, 2 ** 31 - 1], 10
BAD_REPLACED = {0: NMP, 1: -7}
BAD_OUT = dict(held_mp=BAD_HELD, held=[0, 0, 0, 0, 1, 1])


def next_poses(seed=9, B=2):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((2, B, 4))
    q /= np.linalg.norm(q, axis=2)[..., None]
    tracked, prev = (np.concatenate([q[j], rng.uniform(-10, 10, (B, 3))], 1) for j in range(2))
    return tracked, prev
