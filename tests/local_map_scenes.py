"""The scenes of tests/test_local_map_ref.py (CPU: the conditions that keep the GPU tests from passing vacuously) and
tests/test_gpu_local_map.py (GPU: the device against the restatement), with pinned seeds, and the host's side of the sequence
gl_track_frame_chain_map runs on the device.  Test infrastructure; nothing in the product imports it."""
import numpy as np

from gmmloc_amd import api, synth
from tests import chain_glue as G
from tests import local_map_ref as R

# ---- gl_update_local_map: name -> (map seed, NMP, NKF, NFK, B, NF, KFcap, NPcap).  "euroc": the size of a EuRoC session's map; the
# others sit on either side of the two LDS bounds (4 096 key-frames of counters, 1 048 576 map points of mask).
UPDATE_SCENES = {
    "tiny": (11, 300, 40, 24, 16, 50, 64, 256),
    "small": (12, 6000, 150, 300, 24, 400, 128, 4096),
    "euroc_b1": (13, 180000, 1500, 1200, 1, 1200, 256, 16384),
    "euroc_b256": (13, 180000, 1500, 1200, 256, 1200, 256, 16384),
    "kf_at_bound": (14, 30000, 4096, 40, 16, 300, 128, 2048),
    "kf_over_bound": (15, 30000, 4097, 40, 16, 300, 128, 2048),
    "mp_at_bound": (16, 1 << 20, 2000, 600, 16, 600, 128, 16384),
    "mp_over_bound": (17, (1 << 20) + 1, 2000, 600, 16, 600, 128, 16384),
    "both_over_bound": (18, (1 << 20) + 4000, 5000, 300, 16, 600, 128, 16384),
}
BATCHED = [k for k, v in UPDATE_SCENES.items() if v[4] >= 16]


def update_scene(name):
    """-> (map dict, feat_mp (B,NF), lists in: the "previous frame's" values - a short ascending list each, ref_kf = 0)"""
    seed, NMP, NKF, NFK, B, NF, KFcap, NPcap = UPDATE_SCENES[name]
    m = synth.synth_chain_map([], seed, NMP, NKF, NFK)["map"]
    feat_mp = synth.synth_held_points(m, B, NF, seed)
    return m, feat_mp, previous_lists(B, NKF, NMP, KFcap, NPcap)


def previous_lists(B, NKF, NMP, KFcap, NPcap, with_count=True):
    lists = dict(local_kf=np.full((B, KFcap), -7, np.int32), n_local_kf=np.full(B, min(3, NKF, KFcap), np.int32),
                 local_mp=np.full((B, NPcap), -7, np.int32), n_local_mp=np.full(B, min(5, NMP, NPcap), np.int32), ref_kf=np.zeros(B, np.int32),
                 status=np.full(B, -7, np.int32))
    lists["local_kf"][:, :min(3, NKF, KFcap)] = np.arange(min(3, NKF, KFcap))
    lists["local_mp"][:, :min(5, NMP, NPcap)] = np.arange(min(5, NMP, NPcap))
    if with_count:
        lists["kf_count"] = np.full((B, NKF), -7, np.int32)
    return lists


def frame_kinds(m, feat_mp, lists):
    """per frame, from the restatement alone: dict of bool arrays (B,) - new (the list made differs from the one passed in), cleared (an
    invalid held point), invalid_kf (an invalid key-frame with a non-zero count), tie (two valid key-frames share the largest count),
    empty (empty counter)"""
    B = feat_mp.shape[0]
    fm, out = R.update_local_map(m, feat_mp, lists)
    kinds = {k: np.zeros(B, bool) for k in ("new", "cleared", "invalid_kf", "tie", "empty")}
    kfv = np.asarray(m["kf_valid"]) != 0
    for b in range(B):
        r = R.frame_vec(m, feat_mp[b])
        kinds["empty"][b] = r["kept"]
        kinds["cleared"][b] = (fm[b] != feat_mp[b]).any()
        kinds["invalid_kf"][b] = (r["kf_count"][~kfv] > 0).any()
        c = np.where(kfv, r["kf_count"], 0)
        kinds["tie"][b] = c.max() > 0 and (c == c.max()).sum() >= 2
        kinds["new"][b] = not r["kept"] and (out["n_local_mp"][b] != lists["n_local_mp"][b] or
                                              not np.array_equal(out["local_mp"][b], lists["local_mp"][b]))
    return kinds


# ---- gl_track_frame_chain_map: name -> (frames' arguments, map seed, NKF, NFK, KFcap, NPcap)
def _frames(name, cam, scale_factor=1.2):
    F = lambda *a, **kw: synth.synth_chain_frame(*a, scale_factor=scale_factor, **kw)
    if name == "one":  # a frame of the size tools/chain_time.py times
        return [F(1200, 1000, 3000, 7100, cam)]
    if name == "plain":
        return [F(600, 500, 1200, 7200 + b, cam, temporal_frac=(0.3 if b == 1 else 0.0)) for b in range(3)]
    if name == "mixed":  # plain, temporal points, through the key-frame (mode 1), lost (mode 2)
        fs = [F(700, 600, 1400, 7300, cam, NK=500), F(700, 600, 1400, 7301, cam, NK=500, temporal_frac=0.3),
              F(700, 600, 1400, 7302, cam, NK=500, pred_rot_deg=10.0), F(700, 600, 1400, 7303, cam, NK=500, pred_rot_deg=10.0)]
        fs[3]["kf_has_mp"][25:] = 0  # a key-frame with 25 map points: fewer than 10 survive
        return fs
    if name == "fallback_one":
        return [F(700, 600, 1400, 7402, cam, NK=500, pred_rot_deg=10.0)]
    if name == "all_valid":  # no invalid map point: tests/chain_glue.py::check_chain (which knows no clearing) applies
        return [F(700, 600, 1400, 7500 + b, cam, NK=500, temporal_frac=(0.3 if b == 1 else 0.0), pred_rot_deg=(10.0 if b == 2 else None))
                for b in range(3)]
    if name == "branches":  # tests/track_cases.py: 19 matches (tracking.cpp:352; its would-be optimisation has outliers), a
        from tests import oracle_lib, track_cases  # trackWithMotionModel that returns 9 (:53), a frame that tracks (20 matches)
        assert scale_factor == 1.2
        return [track_cases.frame(oracle_lib.load(), n) for n in ("n1_19_s7001", "ret_mm_9", "n1_20_s7001")]
    raise KeyError(name)


CHAIN_SCENES = {"one": (21, 160, 1200, 64, 3328), "plain": (22, 300, 900, 64, 1408), "mixed": (23, 400, 1000, 64, 1600),
                "fallback_one": (24, 160, 1000, 64, 1600), "all_valid": (25, 300, 1000, 64, 1728), "branches": (26, 200, 500, 64, 768)}
WITHOUT_INVALID_POINTS = ("all_valid", "branches")  # (what is compared stage by stage with a checker that knows no clearing)
CHAIN_MODES = {"one": [0], "plain": [0, 0, 0], "mixed": [0, 0, 1, 2], "fallback_one": [1], "all_valid": [0, 0, 1], "branches": [1, 1, 0]}


def chain_scene(name, cam=None, scale_factor=1.2):
    """-> (frames, s = synth_chain_map's dict, lists in (the previous frame's), KFcap, NPcap)"""
    cam = api.Camera() if cam is None else cam
    frames = _frames(name, cam, scale_factor)
    seed, NKF, NFK, KFcap, NPcap = CHAIN_SCENES[name]
    NMP = int(sum(len(f["mp_cand"]) for f in frames) * 1.3) + 64
    s = synth.synth_chain_map(frames, seed, NMP, NKF, NFK, pt_invalid_frac=(0.0 if name in WITHOUT_INVALID_POINTS else 0.04))
    B = len(frames)
    lists = previous_lists(B, NKF, NMP, KFcap, NPcap)
    for b in range(B):
        n, k = min(len(s["prev_local_mp"][b]), NPcap), min(len(s["prev_local_kf"][b]), KFcap)
        lists["local_mp"][b, :n], lists["n_local_mp"][b] = s["prev_local_mp"][b][:n], n
        lists["local_kf"][b, :k], lists["n_local_kf"][b] = s["prev_local_kf"][b][:k], k
    return frames, s, lists, KFcap, NPcap


def host_between_halves(m, f, b, s, fr, lists_in, NP=None):
    """What a host does for frame b between gl_track_frame_chain_front and _back when it follows gl_track_frame_chain_map's sequence:
    feat_mp from the front's associations `fr` (dict of (B, ...) arrays or of one frame's results with the keys match_last, match_kf,
    mode), updateLocalMap (tests/local_map_ref.py), the gather.  NP: slots of the gathered local map (None: NPcap of lists_in; "fit":
    exactly n_local_mp, at least 1).  -> dict(feat_mp, match_last, match_kf, lists (one frame's rows, as arrays of B = 1), local = the
    gathered arrays + to_local tables, NP)"""
    kfm = s["kf_feat_mp"][b]
    fm, ml, mk = R.derive_feat_mp(m, fr["match_last"], fr["match_kf"], s["last_mp"][b], kfm, fr["mode"])
    one = {k: v[b:b + 1] for k, v in lists_in.items()}
    fm2, lists = R.update_local_map(m, fm[None], one)
    assert np.array_equal(fm2[0], fm)  # (derive_feat_mp has cleared every invalid point already)
    NPcap = lists["local_mp"].shape[1]
    n = min(int(lists["n_local_mp"][0]), NPcap)
    NPg = NPcap if NP is None else max(n, 1)
    local = R.gather_local_map(m, lists["local_mp"][0], n, NPg, s["last_mp"][b], kfm)
    return dict(feat_mp=fm, match_last=ml, match_kf=mk, lists=lists, local=local, NP=NPg)


def oracle_sequence(oracle, cam, f, b, s, lists_in):
    """the whole reference sequence of frame b on the CPU oracle: front -> host_between_halves -> stage 3 -> (n3, h, r)"""
    r = G.oracle_front(oracle, cam, f)
    h = host_between_halves(s["map"], f, b, s, dict(match_last=r["match_last"], match_kf=r["match_kf"], mode=r["mode"]), lists_in)
    g = dict(f)
    g.update(h["local"])
    m3, n3, iv = G.oracle_stage3(oracle, cam, g, r["pose"], h["match_last"].astype(np.int64), h["match_kf"].astype(np.int64), r["drop_src"], r["drop_kf"])
    return n3, h, r
