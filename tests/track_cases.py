"""Named frames on both sides of every integer decision Tracking::track makes before trackLocalMap (tests/track_ref.py), for
tests/test_track_ref.py (CPU: every case hits the counts it declares) and tests/test_gpu_track_branches.py.  Test infrastructure.

The decisions and their operands:
  tracking.cpp:345  nmatches < 20 at th = 7   -> the search is run again at th = 14          n7
  tracking.cpp:352  nmatches < 20             -> return before the optimisation              n1
  tracking.cpp:53   num_matches < 10          -> trackKeyFrame                               ret_mm
  tracking.cpp:65   num_matches < 10          -> tracking failure                            ret_kf
  tracking.cpp:305  nmatches < 15             -> a log line: nothing but counts2[1] differs  nbow
Every frame is synth.synth_chain_frame(300, 260, 500, seed, cam, NK = 200) (one: 1200 / 1000 / 3000, whose stage-4 problem is
compacted) edited in numpy; `want` holds the counts the edit aims at, and test_track_ref.py asserts them exactly."""
import functools

import numpy as np

from gmmloc_amd import api, synth
from tests import track_ref as T

NF, NL, NP, NK = 300, 260, 500, 200
FALLBACK_KEYS = ("kf_angle", "kf_desc", "kf_has_mp", "kf_node_id", "kf_node_ptr", "kf_node_idx", "kf_pt", "kf_to_local", "feat_node_id", "feat_node_ptr",
                 "feat_node_idx")


def copy(f):
    return {k: (v.copy() if hasattr(v, "copy") else v) for k, v in f.items()}


def base(seed, shape=(NF, NL, NP), **kw):
    return synth.synth_chain_frame(*shape, seed, api.Camera(), NK=NK, **kw)


def stage1(o, f):
    t = T.Tracking(o, api.Camera(), f)
    n = t._search_last(T.TH_MM)
    if n < 20:
        t.frame.mappoints = [None] * t.NF
        n = t._search_last(2 * T.TH_MM)
    return t.names("last"), n


def trim_n1(o, f, k):
    """exactly k stage-1 matches: the last-frame points of the other matched features are made invalid, until the search agrees"""
    f = copy(f)
    for _ in range(40):
        m, n = stage1(o, f)
        if n <= k:
            break
        idx = np.unique(m[m >= 0])
        f["last_valid"][idx[k:]] = 0
    return f


def trim_ret_mm(o, f, k):
    """all but k of the matches trackWithMotionModel keeps are TEMPORAL points (no observation, not in the local map)"""
    f = copy(f)
    r = T.track(o, api.Camera(), without_fallback(f))
    kept = r["match_last"][r["match_last"] >= 0]
    f["last_observed"][:] = 1
    f["last_observed"][kept[k:]] = 0
    f["last_to_local"] = np.where(f["last_observed"] != 0, f["last_to_local"], -1).astype(np.int32)
    return f


def trim_kf(o, f, k):
    """only k of the key-frame features searchByBoW matched keep their map point"""
    f = copy(f)
    kf = dict(angle=f["kf_angle"], desc=f["kf_desc"], has_mp=f["kf_has_mp"], node_id=f["kf_node_id"], node_ptr=f["kf_node_ptr"], node_idx=f["kf_node_idx"])
    cur = dict(angle=f["feat_angle"], desc=f["feat_desc"], node_id=f["feat_node_id"], node_ptr=f["feat_node_ptr"], node_idx=f["feat_node_idx"])
    m, _ = o.search_by_bow(kf, cur, 0.7, True)
    kk = np.unique(m[m >= 0])
    f["kf_has_mp"][:] = 0
    f["kf_has_mp"][kk[:k]] = 1
    return f


def without_fallback(f):
    return {k: v for k, v in f.items() if k not in FALLBACK_KEYS}


def retry_frame(o, f):
    """fewer than 20 matches at th = 7 only: the prediction is turned until the narrow search fails and the wide one does not"""
    for deg in (1.0, 1.25, 1.5, 1.75, 2.0, 2.5, 3.0):
        g = copy(f)
        a = np.deg2rad(deg)
        dq, q0 = np.array([0, np.sin(a / 2), 0, np.cos(a / 2)]), g["pose_cw"][:4]
        qp = np.concatenate([dq[3] * q0[:3] + q0[3] * dq[:3] + np.cross(dq[:3], q0[:3]), [dq[3] * q0[3] - dq[:3] @ q0[:3]]])
        g["pose_cw"] = np.concatenate([qp, synth.quat_to_R(dq) @ g["pose_cw"][4:]])
        t = T.Tracking(o, api.Camera(), g)
        t.track_with_motion_model()
        if t.n7 < 20 <= t.n1:
            return g
    raise AssertionError("no rotation gives n7 < 20 <= n1")


# name -> (builder(o) -> frame, the counts it aims at)
CASES = {}


def case(name, **want):
    def reg(fn):
        CASES[name] = (fn, want)
        return fn
    return reg


for _seed, _k in ((7000, 9), (7000, 10), (7000, 19), (7000, 20), (7001, 9), (7001, 10), (7001, 19), (7001, 20), (7002, 19)):
    case("n1_%d_s%d" % (_k, _seed), n1=_k)(functools.partial(lambda o, s, k: trim_n1(o, base(s), k), s=_seed, k=_k))
case("retry_to_20_or_more", retried=True, n1_min=20, mode=0)(lambda o: retry_frame(o, base(7003)))
case("ret_mm_9", n1_min=20, ret_mm=9, mode=1)(lambda o: trim_ret_mm(o, base(7100), 9))
case("ret_mm_10", n1_min=20, ret_mm=10, mode=0)(lambda o: trim_ret_mm(o, base(7101), 10))
case("ret_kf_9", ret_kf=9, mode=2)(lambda o: trim_kf(o, base(7100, pred_rot_deg=10.0), 9))
case("ret_kf_10", ret_kf=10, mode=1)(lambda o: trim_kf(o, base(7100, pred_rot_deg=10.0), 10))
case("nbow_14", nbow=14, mode=1)(lambda o: trim_kf(o, base(7101, pred_rot_deg=10.0), 14))
case("nbow_15", nbow=15, mode=1)(lambda o: trim_kf(o, base(7101, pred_rot_deg=10.0), 15))
case("large_n1_19", n1=19)(lambda o: trim_n1(o, base(7200, (1200, 1000, 3000)), 19))
case("large_plain", n1_min=20, mode=0)(lambda o: base(7201, (1200, 1000, 3000)))

BELOW_20 = [n for n, (_, w) in CASES.items() if w.get("n1", 99) < 20]
# the frames of one buffer layout = one batch (neighbouring frames on different branches); the large frame is a batch of its own
LARGE = ["large_n1_19", "large_plain"]
WITH_FALLBACK = [n for n in CASES if n not in LARGE]
NO_FALLBACK = [n for n in CASES if (n.startswith("n1_") and not n.endswith("s7002")) or n.startswith("ret_mm")]

_built = {}


def frame(o, name, fallback=True):
    """the case's frame (built once and never written to again; copy() before editing)"""
    if name not in _built:
        _built[name] = CASES[name][0](o)
    return _built[name] if fallback else without_fallback(_built[name])
