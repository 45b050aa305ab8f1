"""Tracking::updateLocalMap (tracking.cpp:119-207) restated on the flat map arrays of gl_update_local_map - the checker of
tests/test_gpu_local_map.py.  Test infrastructure; nothing in the product imports it.

Written twice: `frame_sets` follows the reference line by line with dicts and sets, `frame_vec` says the same with numpy; both are
kept and compared (tests/test_local_map_ref.py).  The reference's steps, with the quirks that are reproduced:
  1 (:129-145)  per FEATURE with a map point: invalid point -> the feature's map point is cleared; else every observation of the point
                bumps its key-frame's counter (a point held by two features counts twice, a temporal point adds nothing)
  2 (:147-148)  empty counter -> return, everything kept (status 1)
  3 (:150-166)  local key-frames = counted AND valid; ref key-frame = the valid one with the largest count (all invalid: lists empty,
                ref kept)
  4 (:167-181)  the neighbour loop only "adds" key-frames the set already holds: nothing
  5 (:191-206)  local map points = union of the local key-frames' non-null valid map points
The two places where the reference follows unordered_map / unordered_set<pointer> order are fixed canonically, as on the device: a tie
for the reference key-frame goes to the LOWEST row, both lists are in ASCENDING row order.
Malformed input (never produced by a consistent host) is skipped the way the device skips it: a feat_mp / kf_mp entry outside
[-1, NMP) counts nothing and is left alone; a point whose CSR range is not inside [0, NOBS] counts nothing; an observation whose
key-frame is outside [0, NKF) is passed over.

map: dict(obs_ptr (NMP+1,), obs_kf (NOBS,), kf_mp (NKF,NFK), mp_valid (NMP,) or None, kf_valid (NKF,) or None)."""
import numpy as np

KEPT, MP_TRUNCATED, KF_TRUNCATED = 1, 2, 4


def _sizes(m):
    return len(m["obs_ptr"]) - 1, m["kf_mp"].shape[0], m["kf_mp"].shape[1], len(m["obs_kf"])


def frame_sets(m, feat_mp):
    """one frame, dicts and sets -> dict(feat_mp, kept, local_kf, local_mp, ref_kf (None: unchanged), kf_count)"""
    NMP, NKF, NFK, NOBS = _sizes(m)
    mp_valid, kf_valid = m.get("mp_valid"), m.get("kf_valid")
    feat_mp = np.array(feat_mp, np.int32)
    counter = {}
    for i in range(len(feat_mp)):
        p = int(feat_mp[i])
        if p < 0 or p >= NMP:
            continue
        if mp_valid is not None and not mp_valid[p]:
            feat_mp[i] = -1
            continue
        o0, o1 = int(m["obs_ptr"][p]), int(m["obs_ptr"][p + 1])
        if o0 < 0 or o1 < o0 or o1 > NOBS:
            continue
        for o in range(o0, o1):
            k = int(m["obs_kf"][o])
            if 0 <= k < NKF:
                counter[k] = counter.get(k, 0) + 1
    kf_count = np.zeros(NKF, np.int32)
    for k, c in counter.items():
        kf_count[k] = c
    if not counter:
        return dict(feat_mp=feat_mp, kept=True, local_kf=None, local_mp=None, ref_kf=None, kf_count=kf_count)
    best, ref, local = 0, None, set()
    for k in sorted(counter):  # ascending rows: `>` then keeps the lowest row among equal counts
        if kf_valid is not None and not kf_valid[k]:
            continue
        if counter[k] > best:
            best, ref = counter[k], k
        local.add(k)
    # (:167-181 adds nothing)
    pts = set()
    for k in local:
        for p in m["kf_mp"][k]:
            p = int(p)
            if p < 0 or p >= NMP:
                continue
            if mp_valid is not None and not mp_valid[p]:
                continue
            pts.add(p)
    return dict(feat_mp=feat_mp, kept=False, local_kf=np.array(sorted(local), np.int32), local_mp=np.array(sorted(pts), np.int32), ref_kf=ref,
                kf_count=kf_count)


def frame_vec(m, feat_mp):
    """the same, vectorised"""
    NMP, NKF, NFK, NOBS = _sizes(m)
    mp_valid = np.ones(NMP, bool) if m.get("mp_valid") is None else np.asarray(m["mp_valid"]) != 0
    kf_valid = np.ones(NKF, bool) if m.get("kf_valid") is None else np.asarray(m["kf_valid"]) != 0
    feat_mp = np.array(feat_mp, np.int32)
    inr = (feat_mp >= 0) & (feat_mp < NMP)
    p = np.where(inr, feat_mp, 0)
    feat_mp[inr & ~mp_valid[p]] = -1
    held = p[inr & mp_valid[p]].astype(np.int64)
    o0, o1 = m["obs_ptr"][held].astype(np.int64), m["obs_ptr"][held + 1].astype(np.int64)
    ok = (o0 >= 0) & (o1 >= o0) & (o1 <= NOBS)
    o0, n = o0[ok], (o1 - o0)[ok]
    flat = np.repeat(o0, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
    k = np.asarray(m["obs_kf"])[flat].astype(np.int64)
    k = k[(k >= 0) & (k < NKF)]
    kf_count = np.bincount(k, minlength=NKF).astype(np.int32)
    if len(k) == 0:
        return dict(feat_mp=feat_mp, kept=True, local_kf=None, local_mp=None, ref_kf=None, kf_count=kf_count)
    local = np.nonzero((kf_count > 0) & kf_valid)[0].astype(np.int32)
    ref = int(local[np.argmax(kf_count[local])]) if len(local) else None  # (argmax: the first, i.e. lowest, of equal counts)
    pts = np.asarray(m["kf_mp"])[local].ravel()
    pts = pts[(pts >= 0) & (pts < NMP)]
    pts = np.unique(pts[mp_valid[pts]]).astype(np.int32)
    return dict(feat_mp=feat_mp, kept=False, local_kf=local, local_mp=pts, ref_kf=ref, kf_count=kf_count)


def update_local_map(m, feat_mp, lists, frame=frame_vec):
    """B frames on the buffers the device works on: feat_mp (B,NF) and lists = dict(local_kf (B,KFcap), n_local_kf, local_mp (B,NPcap),
    n_local_mp, ref_kf, status[, kf_count (B,NKF)]) are COPIED, updated as gl_update_local_map updates them (a kept frame keeps its lists;
    a truncated list holds its lowest rows and the true count; slots behind a list keep what they held) and returned."""
    feat_mp = np.array(feat_mp, np.int32)
    out = {k: np.array(v, np.int32) for k, v in lists.items()}
    KFcap, NPcap = out["local_kf"].shape[1], out["local_mp"].shape[1]
    for b in range(feat_mp.shape[0]):
        r = frame(m, feat_mp[b])
        feat_mp[b] = r["feat_mp"]
        if "kf_count" in out:
            out["kf_count"][b] = r["kf_count"]
        if r["kept"]:
            out["status"][b] = KEPT
            continue
        nk, npt = len(r["local_kf"]), len(r["local_mp"])
        out["local_kf"][b, :min(nk, KFcap)] = r["local_kf"][:KFcap]
        out["local_mp"][b, :min(npt, NPcap)] = r["local_mp"][:NPcap]
        out["n_local_kf"][b], out["n_local_mp"][b] = nk, npt
        if r["ref_kf"] is not None:
            out["ref_kf"][b] = r["ref_kf"]
        out["status"][b] = (MP_TRUNCATED if npt > NPcap else 0) | (KF_TRUNCATED if nk > KFcap else 0)
    return feat_mp, out


# ---- the host's side of gl_track_frame_chain_map (gmmloc_hip.h, steps 2 and 4), for ONE frame

def derive_feat_mp(m, match_last, match_kf, last_mp, kf_feat_mp, mode):
    """step 2: the map-point row each feature holds after the front half; an invalid held point is cleared in full.  Returns
    (feat_mp, match_last, match_kf) - copies."""
    match_last, match_kf = np.array(match_last, np.int32), np.array(match_kf, np.int32)
    NMP = len(m["obs_ptr"]) - 1
    fm = np.where(match_last >= 0, np.asarray(last_mp)[np.maximum(match_last, 0)],
                  np.where(match_kf >= 0, np.asarray(kf_feat_mp)[np.maximum(match_kf, 0)] if kf_feat_mp is not None else -1, -1)).astype(np.int32)
    if mode == 2:
        fm[:] = -1
    if m.get("mp_valid") is not None:
        inr = (fm >= 0) & (fm < NMP)
        bad = inr & (np.asarray(m["mp_valid"])[np.where(inr, fm, 0)] == 0)
        fm[bad] = -1
        match_kf[bad & (match_last < 0)] = -1
        match_last[bad] = -1
    return fm, match_last, match_kf


def gather_local_map(m, local_mp, n_local_mp, NP, last_mp, kf_feat_mp=None):
    """step 4: the chain's local-map arrays of NP slots from the map's, through the first min(n_local_mp, NP) rows of the ascending list
    (the slots above: zeros, mp_cand = 0), and the to_local tables -> dict of the chain's keys"""
    NMP = len(m["obs_ptr"]) - 1
    n = min(max(int(n_local_mp), 0), NP, len(local_mp))
    rows = np.asarray(local_mp[:n], np.int64)
    on = (rows >= 0) & (rows < NMP)
    g = dict(mp_pos=np.zeros((NP, 3)), mp_normal=np.zeros((NP, 3)), mp_max_dist=np.zeros(NP, np.float32), mp_min_dist=np.zeros(NP, np.float32),
             mp_cand=np.zeros(NP, np.uint8), mp_desc=np.zeros((NP, 32), np.uint8))
    for k in ("mp_pos", "mp_normal", "mp_max_dist", "mp_min_dist", "mp_desc"):
        g[k][:n][on] = m[k][rows[on]]
    g["mp_cand"][:n][on] = 1

    def find(q):
        q = np.asarray(q, np.int64)
        at = np.searchsorted(rows, q)
        hit = (q >= 0) & (at < n) & (rows[np.minimum(at, max(n - 1, 0))] == q) if n else np.zeros(len(q), bool)
        return np.where(hit, at, -1).astype(np.int32)
    g["last_to_local"] = find(last_mp)
    if kf_feat_mp is not None:
        g["kf_to_local"] = find(kf_feat_mp)
    return g
