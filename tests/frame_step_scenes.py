"""The random frames and the synthetic sequence of tests/test_gpu_frame_step.py, with pinned seeds.  Test infrastructure; nothing in the
product imports it."""
import functools

import numpy as np

from gmmloc_amd import api, synth
from tests.ba_window_scenes import _obs_feat

F32 = np.float32
MAP = dict(seed=61, NMP=400, NKF=10, NFK=70)  # a few hundred points, about ten key-frames
TH_DEPTH = 3.5


def ba_of(m, seed, mono_frac=0.2):
    """the gl_map_ba_view arrays the three calls read, for a map of synth.synth_chain_map"""
    rng = np.random.default_rng(seed + 777)
    NKF, NFK = m["kf_mp"].shape
    q = rng.standard_normal((NKF, 4))
    uvr = rng.uniform(0, 480, (NKF, NFK, 3))
    uvr[rng.uniform(size=(NKF, NFK)) < mono_frac, 2] = -1.0
    return dict(kf_pose=np.concatenate([q / np.linalg.norm(q, axis=1)[:, None], rng.uniform(-10, 10, (NKF, 3))], 1), kf_uvr=uvr,
                kf_oct=rng.integers(0, 8, (NKF, NFK)).astype(np.int32), obs_feat=_obs_feat(m), kf_first=0)


@functools.lru_cache(maxsize=None)
def random_map():
    m = synth.synth_chain_map([], MAP["seed"], MAP["NMP"], MAP["NKF"], MAP["NFK"])["map"]
    return m, ba_of(m, MAP["seed"])


def random_end(m, B, NF, seed, NPcap=96):
    """the arguments of frame_end for B frames of NF features (NL = NF) on map m: rows of every kind (observed, without observations,
    invalid, none), local matches up to the last slot, outliers, temporal points, depths on both sides of the range and outside the
    numbers; with B = 3 the frames are tracked, lost, tracked through the key-frame"""
    rng = np.random.default_rng(seed)
    NMP, NKF = len(m["obs_ptr"]) - 1, m["kf_mp"].shape[0]
    feat_mp = np.where(rng.uniform(size=(B, NF)) < 0.6, rng.integers(0, NMP, (B, NF)), -1).astype(np.int32)
    n_local = rng.integers(NPcap // 2, NPcap + 1, B).astype(np.int32)
    local_mp = np.sort(np.stack([rng.choice(NMP, NPcap, replace=False) for _ in range(B)]), 1).astype(np.int32)
    match_local = np.where(rng.uniform(size=(B, NF)) < 0.3, rng.integers(0, n_local[:, None], (B, NF)), -1).astype(np.int32)
    match_last = np.where(feat_mp >= 0, rng.integers(0, NF, (B, NF)), np.where(rng.uniform(size=(B, NF)) < 0.4, rng.integers(0, NF, (B, NF)), -1))
    depth = rng.uniform(-0.5, 2 * TH_DEPTH, (B, NF)).astype(F32)
    depth[rng.uniform(size=(B, NF)) < 0.05] = np.nan
    depth[rng.uniform(size=(B, NF)) < 0.05] = 0.0
    depth[rng.uniform(size=(B, NF)) < 0.05] = TH_DEPTH
    counts2 = np.zeros((B, 4), np.int32)
    counts2[:, 3] = [0, 2, 1][:B] if B <= 3 else rng.integers(0, 3, B)
    return dict(feat_mp=feat_mp, match_last=match_last.astype(np.int32), match_local=match_local, outlier=(rng.uniform(size=(B, NF)) < 0.2).astype(np.uint8),
                local_mp=local_mp, n_local_mp=n_local, counts2=counts2, ref_kf=rng.integers(0, NKF, B).astype(np.int32),
                last_observed=(rng.uniform(size=(B, NF)) < 0.7).astype(np.uint8), feat_depth=depth)


def random_next(m, B, NF, seed, NMPcap=None):
    """the arguments of frame_next: held rows of every kind, new rows at the end of the table (mp_base = NMP - NF // 4), replacements
    of a fifth of the rows (some onto rows that are replaced themselves), poses of a few metres"""
    rng = np.random.default_rng(seed + 5)
    NMP, NKF = len(m["obs_ptr"]) - 1, m["kf_mp"].shape[0]
    NMPcap = NMP + 9 if NMPcap is None else NMPcap
    held = np.where(rng.uniform(size=(B, NF)) < 0.7, rng.integers(0, NMP, (B, NF)), -1).astype(np.int32)
    n_new = max(NF // 4, 1)
    feat_new = -np.ones((B, NF), np.int32)
    for b in range(B):
        at = rng.permutation(NF)
        feat_new[b, at[:n_new]] = rng.permutation(n_new)
        feat_new[b, at[n_new:n_new + max(NF // 10, 1 if NF > 1 else 0)]] = -2
    rep = np.where(rng.uniform(size=NMPcap) < 0.2, rng.integers(0, NMP, NMPcap), -1).astype(np.int32)
    q = rng.standard_normal((2, B, 4))
    q /= np.linalg.norm(q, axis=2)[..., None]
    tracked, prev = (np.concatenate([q[j], rng.uniform(-10, 10, (B, 3))], 1) for j in range(2))
    return dict(pose_tracked=tracked, pose_prev=prev, ref_kf=rng.integers(0, NKF, B).astype(np.int32), held_mp=held, feat_new=feat_new,
                mp_base=NMP - n_new, mp_replaced=rep)


# ---- the sequence: T consecutive non-key frames over one map
SEQ = dict(seed=8100, NF=300, NP=600, NKF=10, NFK=300, T=6)  # (NFK = NF: a frame of the sequence can become a key-frame row)
FRAME_KEYS = ("feat_uv", "feat_ur", "feat_oct", "feat_angle", "feat_desc", "feat_taken", "feat_depth")


def _depth(uv, ur, cam):
    with np.errstate(divide="ignore", invalid="ignore"):
        d = cam.bf / (uv[:, 0] - ur.astype(np.float64))
    return np.where((ur >= 0) & (uv[:, 0] > ur), d, -1.0).astype(F32)


def _se3(q, t):
    return np.concatenate([q, t])


def _compose(d, p):
    """d * p on (qx qy qz qw tx ty tz)"""
    from tests.frame_step_ref import se3_mul
    return se3_mul(np.asarray(d, np.float64), np.asarray(p, np.float64))


def _world_points(f, pose, cam):
    """the point behind every feature with a stereo depth, NaN for the others"""
    d = f["feat_depth"].astype(np.float64)
    uv = f["feat_uv"]
    pc = np.stack([(uv[:, 0] - cam.cx) / cam.fx * d, (uv[:, 1] - cam.cy) / cam.fy * d, d], 1)
    X = (pc - pose[4:]) @ synth.quat_to_R(pose[:4])  # R^T (pc - t)
    return np.where((d > 0)[:, None], X, np.nan)


def follow(prev, X_prev, pose_now, cam, rng, reobs_frac=0.95):
    """the features of a frame at pose_now that re-observes the points X_prev behind the features of `prev` (a dict of FRAME_KEYS):
    sub-pixel noise by octave, a few flipped descriptor bits, a small in-plane rotation; the rest is clutter.  -> (frame, its points:
    the re-observed point, else the one behind the feature's own stereo depth)"""
    NF = len(prev["feat_oct"])
    W, H = cam.width, cam.height
    sf = 1.2 ** np.arange(8)
    Rn, tn = synth.quat_to_R(pose_now[:4]), pose_now[4:]
    src = rng.permutation(NF)
    X = X_prev[src]
    known = np.isfinite(X).all(1)
    pn = np.where(known[:, None], X, 0.0) @ Rn.T + tn
    z = np.where(pn[:, 2] > 0.3, pn[:, 2], 1.0)
    u, v = cam.fx * pn[:, 0] / z + cam.cx, cam.fy * pn[:, 1] / z + cam.cy
    octp = prev["feat_oct"][src]
    ok = known & (octp >= 0) & (pn[:, 2] > 0.3) & (u > 5) & (u < W - 5) & (v > 5) & (v < H - 5) & (rng.uniform(size=NF) < reobs_frac)
    octv = np.where(ok, octp, rng.integers(0, 8, NF)).astype(np.int32)
    uv = np.where(ok[:, None], np.stack([u, v], 1) + rng.normal(0, 0.4, (NF, 2)) * sf[octv][:, None],
                  np.stack([rng.uniform(5, W - 5, NF), rng.uniform(5, H - 5, NF)], 1))
    zf = np.where(ok, z, rng.uniform(1.5, 8.0, NF))
    uv = synth._key_point_uv(uv, True)
    ur = np.where(rng.uniform(size=NF) < 0.85, uv[:, 0] - cam.bf / zf + rng.normal(0, 0.3, NF) * sf[octv], -1.0).astype(F32)
    angle = np.where(ok, (prev["feat_angle"][src] - 1.0 + rng.normal(0, 2, NF)) % 360.0, rng.uniform(0, 360, NF)).astype(F32)
    desc = np.where(ok[:, None], prev["feat_desc"][src], rng.integers(0, 256, (NF, 32), dtype=np.uint8)).astype(np.uint8)
    for i in np.nonzero(ok)[0]:
        bits = rng.choice(256, int(rng.integers(0, 9)), replace=False)
        np.bitwise_xor.at(desc[i], bits // 8, (1 << (bits % 8)).astype(np.uint8))
    f = dict(feat_uv=uv, feat_ur=ur, feat_oct=octv, feat_angle=angle, feat_desc=desc, feat_taken=np.zeros(NF, np.uint8), feat_depth=_depth(uv, ur, cam))
    return f, np.where(ok[:, None], X, _world_points(f, pose_now, cam))


@functools.lru_cache(maxsize=None)
def sequence():
    """-> dict(cam, frames: T dicts of FRAME_KEYS (one frame each, no batch axis), first: the chain's last-frame inputs of frame 0 +
    last_mp, s: synth_chain_map's dict (the map), ba, lists: the previous frame's lists, KFcap, NPcap, poses: the true Tcw)"""
    from tests import local_map_scenes as LS
    cam = api.Camera()
    g = SEQ
    f0 = synth.synth_chain_frame(g["NF"], g["NF"], g["NP"], g["seed"], cam)
    NMP = int(g["NP"] * 1.3) + 64
    s = synth.synth_chain_map([f0], g["seed"], NMP, g["NKF"], g["NFK"], window=4)
    rng = np.random.default_rng(g["seed"] + 1)
    frames = [dict({k: f0[k] for k in FRAME_KEYS[:-1]}, feat_depth=_depth(f0["feat_uv"], f0["feat_ur"], cam))]
    ang = np.deg2rad(0.4)
    delta = _se3(np.array([0.0, np.sin(ang / 2), 0.0, np.cos(ang / 2)]), np.array([0.012, -0.004, -0.015]))
    poses = [np.asarray(f0["pose_true"], np.float64)]
    X = _world_points(frames[0], poses[0], cam)
    for t in range(1, g["T"]):
        poses.append(_compose(delta, poses[-1]))
        f, X = follow(frames[-1], X, poses[-1], cam, rng)
        frames.append(f)
    KFcap, NPcap = 16, 896
    lists = LS.previous_lists(1, g["NKF"], NMP, KFcap, NPcap)
    n, k = min(len(s["prev_local_mp"][0]), NPcap), min(len(s["prev_local_kf"][0]), KFcap)
    lists["local_mp"][0, :n], lists["n_local_mp"][0] = s["prev_local_mp"][0][:n], n
    lists["local_kf"][0, :k], lists["n_local_kf"][0] = s["prev_local_kf"][0][:k], k
    first = {k: f0[k] for k in ("pose_lw", "pose_cw", "last_pt", "last_valid", "last_observed", "last_oct", "last_angle", "last_desc")}
    first["last_mp"] = s["last_mp"][0]
    return dict(cam=cam, frames=frames, first=first, s=s, ba=ba_of(s["map"], g["seed"]), lists=lists, KFcap=KFcap, NPcap=NPcap, poses=poses)
