"""Hand-built cases for the found / visible counters and removeMapPoints (gl_map_stats_*, gl_cull_map_points), one on either side of
every decision, with every output DECLARED here: tests/test_map_stats_ref.py shows that the sequential model of tests/map_stats_ref.py
gives them, tests/test_gpu_map_stats.py that the device does.  Test infrastructure; nothing in the product imports it.

The float32 facts the ratio rows rest on (numpy float32, round to nearest even):
  1 / 4 = 0.25 exactly; 1 / 5 < 0.25
  4194303 / 16777212 = 0.25 exactly (both convert exactly)
  16777217 -> 2^24 as a float, so 4194304 / 16777217 = 0.25: KEPT although the exact ratio is below 0.25
  16777218 is a float: 4194304 / 16777218 = 0.24999997
  16777219 -> 2^24 + 4;  8388607 / 33554431 -> 8388607 / 2^25 < 0.25
  0 / 0 = NaN and 1 / 0 = inf: neither is below 0.25f, the entry falls through to the age branches"""
import numpy as np

NKF, NFK = 8, 24
KF_ROW = 5  # curr_kf_: curr_idx = 5 with kf_idx NULL
S, M = True, False  # a stereo observation (weight 2), a monocular one (weight 1)

# name: (found, visible, ref_idx, observations as stereo flags (one key-frame each, rows 0, 1, 2, ...), valid, the verdict of removeMapPoints)
POINTS = [
    ("ratio_1_4", 1, 4, 5, (S, S), 1, 0),
    ("ratio_1_5", 1, 5, 5, (S, S), 1, 2),
    ("ratio_exact_quarter", 4194303, 16777212, 5, (S, S), 1, 0),
    ("ratio_visible_rounds_down", 4194304, 16777217, 5, (S, S), 1, 0),
    ("ratio_just_below", 4194304, 16777218, 5, (S, S), 1, 2),
    ("ratio_visible_rounds_up", 4194304, 16777219, 5, (S, S), 1, 2),
    ("ratio_2p25", 8388607, 33554431, 5, (S, S), 1, 2),
    ("nan_young", 0, 0, 5, (S, S), 1, 0),
    ("nan_age2_weight3", 0, 0, 3, (S, M), 1, 3),
    ("inf_age3_weight4", 1, 0, 2, (S, S), 1, 4),
    ("age1_weight3", 1, 1, 4, (S, M), 1, 0),
    ("age2_weight3_stereo_mono", 1, 1, 3, (S, M), 1, 3),
    ("age2_weight4_two_stereo", 1, 1, 3, (S, S), 1, 0),
    ("age3_weight4_four_mono", 1, 1, 2, (M, M, M, M), 1, 4),
    ("age2_weight3_three_mono", 1, 1, 3, (M, M, M), 1, 3),
    ("age3_weight3", 1, 1, 2, (S, M), 1, 3),
    ("ref_idx_default", 1, 1, -1, (S, S), 1, 4),
    ("invalid", 1, 1, 5, (), 0, 1),
    ("age2_weight4_four_mono", 1, 1, 3, (M, M, M, M), 1, 0),
    ("age3_weight5", 1, 1, 2, (S, S, M), 1, 4),
]
NMP = len(POINTS)
ROW = {p[0]: i for i, p in enumerate(POINTS)}

# ---- the candidate lists: (list, verdict per entry, the list afterwards, rm_mp)
_ALL = list(range(NMP))
LISTS = {
    # every point once, then: a removed row again (finds not_valid_), a kept row again (both stay), rows -1 and NMP, an aged row again
    "decisions": (_ALL + [1, 0, -1, NMP, 13, 11],
                  [0, 2, 0, 0, 2, 2, 2, 0, 3, 4, 0, 3, 0, 4, 3, 3, 4, 1, 0, 4] + [1, 0, 5, 5, 4, 1],
                  [0, 2, 3, 7, 10, 12, 18, 0],
                  [1, 4, 5, 6, 8, 11, 14, 15]),
    "empty": ([], [], [], []),
    "all_removed": ([15, 1, 14, 4, 11], [3, 2, 3, 2, 3], [], [15, 1, 14, 4, 11]),
    "none_removed": ([18, 0, 12, 2, 3, 7, 10], [0] * 7, [18, 0, 12, 2, 3, 7, 10], []),
    "twice_kept_twice_removed": ([12, 5, 12, 5, 5], [0, 2, 0, 1, 1], [12, 12], [5]),
}
# result[2] = erased without removal, result[3]: STATUS_BAD_ROW where a row is outside the table
BAD_ROW_LISTS = ("decisions",)

# kf_idx that is NOT the identity: idx_ = 100 + row; the same points with ref_idx + 100 (the default -1 stays) give the same verdicts
KF_IDX_SHIFT = 100
# the subtraction in 64 bits: curr_idx = kf_idx[KF_ROW] = 2^31 - 1
WIDE_KF_IDX = [0, 1, 2, 3, 4, 2 ** 31 - 1, 6, 7]
WIDE_POINTS = [  # (ref_idx, verdict), every one with found = visible = 1 and weight 4
    (-2 ** 31, 4),  # age 2^32 - 1 (a 32-bit subtraction wraps to -1: kept)
    (2 ** 31 - 3, 0),  # age 2
    (2 ** 31 - 4, 4),  # age 3
    (2 ** 31 - 1, 0),  # age 0
]


def build_map(points, nkf=NKF, nfk=NFK):
    """points: per point (valid, stereo flags) -> (m, ba): observation j of a point is by key-frame row j, at the next free feature"""
    kf_mp = -np.ones((nkf, nfk), np.int32)
    uvr = np.zeros((nkf, nfk, 3), np.float64)
    uvr[:, :, 2] = -1.0
    used = [0] * nkf
    ptr, okf, ofeat = [0], [], []
    for p, (valid, obs) in enumerate(points):
        for k, stereo in enumerate(obs):
            f = used[k]
            used[k] += 1
            assert f < nfk
            kf_mp[k, f] = p
            uvr[k, f] = (10.0 + f, 20.0 + k, 5.0 if stereo else -1.0)
            okf.append(k)
            ofeat.append(f)
        ptr.append(len(okf))
    m = dict(mp_valid=np.array([v for v, _ in points], np.uint8), kf_valid=np.ones(nkf, np.uint8), kf_mp=kf_mp, obs_ptr=np.array(ptr, np.int32),
             obs_kf=np.array(okf, np.int32))
    ba = dict(kf_uvr=uvr, kf_oct=np.zeros((nkf, nfk), np.int32), obs_feat=np.array(ofeat, np.int32), kf_first=-1)
    return m, ba


def cull_scene(variant="rows"):
    """-> dict(m, ba, visible, found, ref_idx, kf_idx) for variant 'rows' (kf_idx None), 'shifted' or 'wide'"""
    if variant == "wide":
        m, ba = build_map([(1, (S, S))] * len(WIDE_POINTS))
        n = len(WIDE_POINTS)
        return dict(m=m, ba=ba, visible=np.ones(n, np.int32), found=np.ones(n, np.int32), ref_idx=np.array([r for r, _ in WIDE_POINTS], np.int32),
                    kf_idx=np.array(WIDE_KF_IDX, np.int32))
    m, ba = build_map([(p[5], p[4]) for p in POINTS])
    ref = np.array([p[3] for p in POINTS], np.int32)
    kf_idx = None
    if variant == "shifted":
        ref = np.where(ref >= 0, ref + KF_IDX_SHIFT, ref).astype(np.int32)
        kf_idx = (np.arange(NKF) + KF_IDX_SHIFT).astype(np.int32)
    return dict(m=m, ba=ba, visible=np.array([p[2] for p in POINTS], np.int32), found=np.array([p[1] for p in POINTS], np.int32), ref_idx=ref,
                kf_idx=kf_idx)


WIDE_LIST = ([0, 1, 2, 3], [v for _, v in WIDE_POINTS], [1, 3], [])

# ---- merge: (visible, found, src, tgt) -> (visible, found), the walk in step order
I32_MAX = 2 ** 31 - 1
MERGE = dict(
    NMP=8,
    visible=[1, 2, 3, 4, I32_MAX, 1, 7, 8], found=[10, 20, 30, 40, 50, 60, 70, 80],
    #     a->b  b->c  c->c  outside  outside  two more steps into c   c->a    wraps
    src=[0, 1, 3, -1, 5, 6, 7, 2, 4],
    tgt=[1, 2, 3, 4, 8, 2, 2, 0, 5],
    # 0->1: (3, 30); 1->2: (6, 60); 6->2: (13, 130); 7->2: (21, 210); 2->0: (22, 220); 4->5: 1 + (2^31 - 1) wraps
    visible_out=[22, 3, 21, 4, I32_MAX, -2 ** 31, 7, 8], found_out=[220, 30, 210, 40, 50, 110, 70, 80],
)

# ---- track: B = 3 frames of NF = 8 features on a local map of NPcap = 4 slots, NMP = 10, every counter 1 on entry
TRACK = dict(
    NMP=10,
    # frame 0: row 3 held by two features; features 2 (its invalid point un-held by the chain) and 4 (a temporal point) hold no row;
    #          feature 3 holds row 5 and is an outlier; feature 5 matched slot 0 (row 1, inlier), feature 7 slot 2 (row 6, outlier);
    #          n_local_mp = 6 > NPcap: the slots end at NPcap; slots 0, 2, 3 in view
    # frame 1: LOST (counts2[3] = 2): the same arrays add nothing
    # frame 2: shares rows 3, 1, 7 with frame 0; feature 3's match_local is beyond NPcap, feature 7 holds a row outside the table; slot 2
    #          holds -1, slot 3 is behind n_local_mp = 3
    feat_mp=[[3, 3, -1, 5, -1, -1, 7, -1], [3, 3, -1, 5, -1, -1, 7, -1], [3, 1, -1, -1, -1, -1, -1, 12]],
    match_local=[[-1, -1, -1, -1, -1, 0, -1, 2], [-1, -1, -1, -1, -1, 0, -1, 2], [-1, -1, 0, 9, -1, -1, -1, -1]],
    outlier=[[0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0, 1, 0, 0, 0, 1], [0, 1, 0, 0, 0, 0, 0, 0]],
    local_mp=[[1, 2, 6, 9], [1, 2, 6, 9], [7, 3, -1, 11]],
    inview=[[1, 0, 1, 1], [1, 0, 1, 1], [1, 0, 1, 1]],
    n_local_mp=[6, 6, 3],
    counts2=[[25, 0, 0, 0], [3, 0, 0, 2], [4, 30, 12, 1]],
    visible_out=[1, 3, 1, 4, 1, 2, 2, 3, 1, 2], found_out=[1, 2, 1, 4, 1, 1, 1, 3, 1, 1],
)


def track_arrays():
    t = TRACK
    return dict(feat_mp=np.array(t["feat_mp"], np.int32), match_local=np.array(t["match_local"], np.int32), outlier=np.array(t["outlier"], np.uint8),
                inview=np.array(t["inview"], np.uint8), local_mp=np.array(t["local_mp"], np.int32), n_local_mp=np.array(t["n_local_mp"], np.int32),
                counts2=np.array(t["counts2"], np.int32))


def random_case(sc, rng, n):
    """counters, ages and a list with duplicates, invalid rows and rows outside the table"""
    m = sc["m"]
    NMP, NKF = len(m["mp_valid"]), len(m["kf_valid"])
    visible = rng.integers(0, 12, NMP).astype(np.int32)
    found = rng.integers(0, 6, NMP).astype(np.int32)
    kf_row = int(rng.integers(0, NKF))
    kf_idx = np.sort(rng.choice(3 * NKF, NKF, replace=False)).astype(np.int32) if rng.random() < 0.5 else None
    curr = kf_row if kf_idx is None else int(kf_idx[kf_row])
    ref_idx = (curr - rng.integers(-1, 5, NMP)).astype(np.int32)
    ref_idx[rng.random(NMP) < 0.05] = -1
    pool = rng.choice(NMP, max(n // 2, 1))
    cand = rng.choice(pool, n).astype(np.int32) if n else np.zeros(0, np.int32)
    if n > 4:
        cand[rng.integers(0, n, 2)] = (-1, NMP)
    return dict(visible=visible, found=found, ref_idx=ref_idx, kf_idx=kf_idx, kf_row=kf_row, cand=cand)
