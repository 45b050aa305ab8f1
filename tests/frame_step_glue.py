"""gl_track_frame_end, gl_map_note_replaced and gl_track_frame_next said a second time, vectorised over rows in numpy: what the device
does (include/gmmloc_hip.h), malformed rows included.  tests/test_frame_step_cases.py holds it to the sequential object model of
tests/frame_step_ref.py and to declared outputs; the GPU tests hold the device to both.  Test infrastructure; nothing in the product
imports it."""
import numpy as np

from tests.frame_step_ref import BAD_REF, F32, KF_INTERRUPT_BA, KF_NEED, se3_inverse, se3_load, se3_mul


def _sizes(m):
    return len(m["obs_ptr"]) - 1, m["kf_mp"].shape[0], m["kf_mp"].shape[1], len(m["obs_kf"])


def in_table(rows, n):
    rows = np.asarray(rows, np.int64)
    return (rows >= 0) & (rows < n)


def observed(m, rows):
    """per entry of `rows`: inside [0, NMP) and its CSR range a non-empty sub-range of [0, NOBS]"""
    NMP, _, _, NOBS = _sizes(m)
    ok = in_table(rows, NMP)
    r = np.where(ok, rows, 0).astype(np.int64)
    ptr = np.asarray(m["obs_ptr"], np.int64)
    a, b = ptr[r], ptr[r + 1]
    return ok & (a >= 0) & (b > a) & (b <= NOBS)


def weighted_count(m, ba, rows):
    """the weighted count (gl_cull_keyframes) per entry of `rows` inside the table; 0 outside and for a malformed range"""
    NMP, NKF, NFK, NOBS = _sizes(m)
    ptr, okf, ofeat, uvr = np.asarray(m["obs_ptr"], np.int64), np.asarray(m["obs_kf"], np.int64), np.asarray(ba["obs_feat"], np.int64), np.asarray(ba["kf_uvr"])
    ok_o = (okf >= 0) & (okf < NKF) & (ofeat >= 0) & (ofeat < NFK)
    w_o = np.where(ok_o, np.where(uvr[np.where(ok_o, okf, 0), np.where(ok_o, ofeat, 0), 2] >= 0, 2, 1), 0) if NOBS else np.zeros(0, np.int64)
    cum = np.concatenate([[0], np.cumsum(w_o)])
    rows = np.asarray(rows, np.int64)
    ok = in_table(rows, NMP)
    r = np.where(ok, rows, 0)
    a, b = ptr[r], ptr[r + 1]
    good = ok & (a >= 0) & (b >= a) & (b <= NOBS)
    return np.where(good, cum[np.where(good, b, 0)] - cum[np.where(good, a, 0)], 0)


def frame_end(m, ba, feat_mp, match_last, match_local, outlier, local_mp, n_local_mp, counts2, ref_kf, last_observed, feat_depth, th_depth, rule=None,
              poison=None):
    """-> dict(held_mp, held, stat, ratio_map).  match_last and last_observed are not read: a temporal point leaves no trace."""
    feat_mp, match_local, outlier, local_mp = (np.asarray(a) for a in (feat_mp, match_local, outlier, local_mp))
    B, NF = feat_mp.shape
    NMP, NKF, NFK, _ = _sizes(m)
    NPcap = local_mp.shape[1]
    out = dict(held_mp=np.full((B, NF), -1, np.int32), held=np.zeros((B, NF), np.uint8), stat=np.zeros((B, 8), np.int32), ratio_map=np.zeros(B, F32))
    if poison is not None:
        out = {k: np.array(poison[k]) for k in out}
    valid = np.ones(NMP, bool) if m.get("mp_valid") is None else np.asarray(m["mp_valid"]) != 0
    depth = np.asarray(feat_depth, F32)
    for b in range(B):
        mode = 0 if counts2 is None else int(counts2[b][3])
        if mode == 2:
            out["stat"][b] = [0, 10, 0, 0, 0, 0, 0, 0]
            continue
        nl = min(max(int(n_local_mp[b]), 0), NPcap)
        j = match_local[b].astype(np.int64)
        use = (j >= 0) & (j < nl)
        r = np.where(use, local_mp[b][np.where(use, j, 0)] if NPcap else -1, feat_mp[b])
        keep = observed(m, r) & (np.asarray(outlier[b]) == 0)
        with np.errstate(invalid="ignore"):
            in_depth = (depth[b] > F32(0)) & (depth[b] < F32(th_depth))
        nmi, num_map, num_total = int(keep.sum()), int((keep & in_depth).sum()), int(in_depth.sum())
        ratio = F32(num_map) / F32(max(1, num_total))
        nref = verdict = 0
        if rule is not None:
            k = int(ref_kf[b])
            if 0 <= k < NKF:
                p = np.asarray(m["kf_mp"][k], np.int64)
                ok = in_table(p, NMP)
                ok &= valid[np.where(ok, p, 0)]
                nref = int((ok & (weighted_count(m, ba, p) >= (2 if rule["num_kfs"] <= 2 else 3))).sum())
            th_ref = F32(0.4) if rule["num_kfs"] < 2 else F32(0.75)
            th_map = F32(0.2) if nmi > 300 else F32(0.35)
            c1a = F32(rule["frame_idx"]) >= F32(rule["kf_frame_idx"]) + F32(rule["fps"])
            c1b = F32(nmi) < F32(nref) * F32(0.25) or ratio < F32(0.3)
            c2 = (F32(nmi) < F32(nref) * th_ref or ratio < th_map) and nmi > 15
            if (c1a or c1b or rule["is_idle"]) and c2:
                verdict = KF_NEED if rule["is_idle"] else KF_INTERRUPT_BA | (KF_NEED if rule["n_queue"] < 3 else 0)
        out["held_mp"][b] = np.where(keep, r, -1)
        out["held"][b] = keep
        out["stat"][b] = [int(mode == 0), nmi, num_map, num_total, nref, verdict, 0, 0]
        out["ratio_map"][b] = ratio
    return out


def note_replaced(mp_replaced, src, tgt, n=None):
    """the last valid step per source wins"""
    rep = np.array(mp_replaced, np.int32)
    n = len(src) if n is None else min(max(int(n), 0), len(src))
    s, t = np.asarray(src[:n], np.int64), np.asarray(tgt[:n], np.int64)
    ok = in_table(s, len(rep)) & in_table(t, len(rep)) & (s != t)
    s, t = s[ok], t[ok]
    if len(s):
        uniq, first_rev = np.unique(s[::-1], return_index=True)  # the first occurrence from the back = the last step
        rep[uniq] = t[::-1][first_rev]
    return rep


def frame_next(m, ba, pose_tracked, pose_prev, ref_kf, held_mp, feat_new=None, mp_base=0, mp_replaced=None, dtype=np.float64, poison=None):
    """-> dict(t_rc, t_cr, pose_lw, pose_cw, held_mp, last_pt, last_valid, last_observed, held, status[, last_desc with m['mp_desc']]);
    poison: the outputs as they stand before the call (the poses of a frame whose ref_kf is outside the table, the descriptors of the
    slots without a row)"""
    held_mp = np.asarray(held_mp)
    B, NF = held_mp.shape
    NMP, NKF, _, _ = _sizes(m)
    out = dict(t_rc=np.zeros((B, 7), dtype), t_cr=np.zeros((B, 7), dtype), pose_lw=np.zeros((B, 7), dtype), pose_cw=np.zeros((B, 7), dtype))
    if poison is not None:
        out = {k: np.array(poison[k], dtype) if k in poison else v for k, v in out.items()}
    h = held_mp.astype(np.int64)
    if feat_new is not None:
        fn = np.asarray(feat_new, np.int64)
        new = fn + int(mp_base)
        h = np.where((fn >= 0) & in_table(new, NMP), new, np.where(fn == -2, -1, h))
    if mp_replaced is not None:
        ok = in_table(h, NMP)
        rep = np.asarray(mp_replaced, np.int64)[np.where(ok, h, 0)]
        h = np.where(ok & in_table(rep, NMP), rep, h)
    row = in_table(h, NMP)
    obs = observed(m, h)
    out.update(held_mp=h.astype(np.int32), last_pt=np.where(row[..., None], np.asarray(m["mp_pos"])[np.where(row, h, 0)], 0.0),
               last_valid=row.astype(np.uint8), last_observed=obs.astype(np.uint8), held=np.where(~row, 0, np.where(obs, 1, 2)).astype(np.uint8),
               status=np.zeros(B, np.int32))
    if m.get("mp_desc") is not None:
        base = np.zeros((B, NF, 32), np.uint8) if poison is None or poison.get("last_desc") is None else np.array(poison["last_desc"])
        out["last_desc"] = np.where(row[..., None], np.asarray(m["mp_desc"])[np.where(row, h, 0)], base)
    for b in range(B):
        k = int(ref_kf[b])
        if not 0 <= k < NKF:
            out["status"][b] = BAD_REF
            continue
        Tkw, Tcw = se3_load(ba["kf_pose"][k], dtype), se3_load(pose_tracked[b], dtype)
        Trc = se3_mul(Tkw, se3_inverse(Tcw))
        Tcr = se3_inverse(Trc)
        lw = se3_mul(Tcr, Tkw)
        cw = lw if pose_prev is None else se3_mul(se3_mul(lw, se3_inverse(se3_load(pose_prev[b], dtype))), lw)
        out["t_rc"][b], out["t_cr"][b], out["pose_lw"][b], out["pose_cw"][b] = Trc, Tcr, lw, cw
    return out


def temporal_last_mp(held_mp, held, feat_depth, th_depth):
    """gl_create_temporal_points on frame_next's rows, the part that bears on last_mp -> (temp_flag, last_mp): the slots with depth > 0 in
    (depth, index) order up to and with the first whose depth is above th_depth at a position past 100 are walked; a walked slot whose
    held is not 1 gets a temporal point and last_mp = -1, every other entry keeps its value"""
    held_mp, held, depth = np.asarray(held_mp), np.asarray(held), np.asarray(feat_depth, F32)
    flag = np.zeros(held.shape, np.uint8)
    for b in range(held.shape[0]):
        idx = np.nonzero(depth[b] > 0)[0]
        idx = idx[np.lexsort((idx, depth[b][idx]))]
        stop = np.nonzero((depth[b][idx] > F32(th_depth)) & (np.arange(len(idx)) + 1 > 100))[0]
        walked = idx if len(stop) == 0 else idx[:stop[0] + 1]
        flag[b, walked[held[b][walked] != 1]] = 1
    return flag, np.where(flag != 0, -1, held_mp).astype(np.int32)
