"""KeyFrame::updateConnections (keyframe.cpp:243-316) and the window selection + flattening of Localization::jointOptimization
(localization_opt.cpp:460-516, :639-763) restated on the flat map arrays of gl_update_connections / gl_ba_window_build, and the
write-back of gl_ba_window_apply - the checker of tests/test_gpu_ba_window.py.  Test infrastructure; nothing in the product imports it.

Written twice: `connections_seq` / `window_seq` follow the reference line by line, with its marks ba_local_kf_ / fixed_kf_idx_ba (and the
map points' ba_local_kf_) kept as arrays; `connections_vec` / `window_vec` say the same with numpy.  Both are kept and compared
(tests/test_ba_window_ref.py).  The one place where the reference follows pointer values - the order of equal weights in
ordered_keyframes_, and which of several largest counts is pKFmax - is fixed canonically, as on the device: the LOWEST key-frame row
first.  fixcam_obs / best_obs (:492, :509-530) are dead (flag_fixsingle is false at :585) and do not appear.
Malformed input is skipped the way the device skips it: kf_mp / obs_kf rows outside the tables, a CSR range that is not inside
[0, NOBS] (no observation), an observation whose feature index is outside [0, NFK) (that observation alone).
A point that ends without an edge (no observation by a valid key-frame, mp_assoc < 0) is dropped from the window and counted.

map: the dict of tests/local_map_ref.py + mp_pos; ba: dict(kf_pose (NKF,7), kf_uvr (NKF,NFK,3), kf_oct (NKF,NFK), obs_feat (NOBS,),
mp_assoc (NMP,), kf_first int[, kf_twc (NKF,3)])."""
import numpy as np

TH = 15
CONN_KEPT, CONN_TRUNCATED, CONN_BAD_ROW = 1, 2, 4
NO_CONN, P_TRUNC, F_TRUNC, L_TRUNC, O_TRUNC, BAD_ROW = 1, 2, 4, 8, 16, 32
TRUNCATED, DROPPED_SHIFT = 30, 8


def _sizes(m):
    return len(m["obs_ptr"]) - 1, m["kf_mp"].shape[0], m["kf_mp"].shape[1], len(m["obs_kf"])


def _valid(m):
    NMP, NKF, _, _ = _sizes(m)
    mpv = np.ones(NMP, bool) if m.get("mp_valid") is None else np.asarray(m["mp_valid"]) != 0
    kfv = np.ones(NKF, bool) if m.get("kf_valid") is None else np.asarray(m["kf_valid"]) != 0
    return mpv, kfv


def _range(m, p, NOBS):
    o0, o1 = int(m["obs_ptr"][p]), int(m["obs_ptr"][p + 1])
    return (o0, o1) if 0 <= o0 <= o1 <= NOBS else (0, 0)


# ---- KeyFrame::updateConnections

def connections_seq(m, kf):
    """-> dict(kf_count (NKF,), empty, conn_kf, conn_w) - the lists in full"""
    NMP, NKF, NFK, NOBS = _sizes(m)
    mpv, _ = _valid(m)
    counter = {}
    for p in m["kf_mp"][kf]:  # (:253-272)
        p = int(p)
        if p < 0 or p >= NMP or not mpv[p]:
            continue
        o0, o1 = _range(m, p, NOBS)
        for o in range(o0, o1):
            k = int(m["obs_kf"][o])
            if k < 0 or k >= NKF or k == kf:
                continue
            counter[k] = counter.get(k, 0) + 1
    kf_count = np.zeros(NKF, np.int32)
    for k, c in counter.items():
        kf_count[k] = c
    if not counter:  # (:275-276)
        return dict(kf_count=kf_count, empty=True, conn_kf=np.zeros(0, np.int32), conn_w=np.zeros(0, np.int32))
    nmax, kmax, pairs = 0, None, []
    for k in sorted(counter):  # ascending rows: `>` keeps the lowest row among equal counts
        if counter[k] > nmax:
            nmax, kmax = counter[k], k
        if counter[k] >= TH:
            pairs.append((counter[k], k))
    if not pairs:
        pairs.append((nmax, kmax))
    pairs.sort(key=lambda wk: (-wk[0], wk[1]))  # (:302-308 sorts ascending and pushes to the front: descending weight; ties -> lowest row)
    return dict(kf_count=kf_count, empty=False, conn_kf=np.array([k for _, k in pairs], np.int32), conn_w=np.array([w for w, _ in pairs], np.int32))


def connections_vec(m, kf):
    NMP, NKF, NFK, NOBS = _sizes(m)
    mpv, _ = _valid(m)
    p = np.asarray(m["kf_mp"][kf]).astype(np.int64)
    p = p[(p >= 0) & (p < NMP)]
    p = p[mpv[p]]
    o0, o1 = m["obs_ptr"][p].astype(np.int64), m["obs_ptr"][p + 1].astype(np.int64)
    ok = (o0 >= 0) & (o1 >= o0) & (o1 <= NOBS)
    o0, n = o0[ok], (o1 - o0)[ok]
    flat = np.repeat(o0, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
    k = np.asarray(m["obs_kf"])[flat].astype(np.int64)
    k = k[(k >= 0) & (k < NKF) & (k != kf)]
    kf_count = np.bincount(k, minlength=NKF).astype(np.int32)
    if len(k) == 0:
        return dict(kf_count=kf_count, empty=True, conn_kf=np.zeros(0, np.int32), conn_w=np.zeros(0, np.int32))
    keep = np.nonzero(kf_count >= TH)[0]
    if len(keep) == 0:
        keep = np.array([np.argmax(kf_count)])  # (the first, i.e. lowest, of equal counts)
    keep = keep[np.lexsort((keep, -kf_count[keep].astype(np.int64)))]
    return dict(kf_count=kf_count, empty=False, conn_kf=keep.astype(np.int32), conn_w=kf_count[keep])


def update_connections(m, kf_rows, out, conn=connections_vec):
    """B key-frames on the buffers the device works on: out = dict(conn_kf (B,Ccap), conn_w (B,Ccap), n_conn, status[, kf_count]) is
    COPIED, updated as gl_update_connections updates it and returned"""
    out = {k: np.array(v, np.int32) for k, v in out.items()}
    NKF = m["kf_mp"].shape[0]
    Ccap = out["conn_kf"].shape[1]
    for b, kf in enumerate(kf_rows):
        kf = int(kf)
        if kf < 0 or kf >= NKF:
            out["n_conn"][b], out["status"][b] = 0, CONN_BAD_ROW
            if "kf_count" in out:
                out["kf_count"][b] = 0
            continue
        r = conn(m, kf)
        if "kf_count" in out:
            out["kf_count"][b] = r["kf_count"]
        n = len(r["conn_kf"])
        out["n_conn"][b] = n
        if r["empty"]:
            out["status"][b] = CONN_KEPT
            continue
        out["conn_kf"][b, :min(n, Ccap)] = r["conn_kf"][:Ccap]
        out["conn_w"][b, :min(n, Ccap)] = r["conn_w"][:Ccap]
        out["status"][b] = CONN_TRUNCATED if n > Ccap else 0
    return out


# ---- Localization::jointOptimization, :460-516 and :639-763

def _pack(m, ba, kf, no_conn, local_kfs, fixed_kfs, pts, obs_of, dropped):
    """the flat window from the lists: obs_of[i] = the CSR positions kept for point i"""
    order = np.array(list(local_kfs) + list(fixed_kfs), np.int32)
    index = {int(k): j for j, k in enumerate(order)}
    P, F, L = len(local_kfs), len(fixed_kfs), len(pts)
    win_obs = np.array([o for os_ in obs_of for o in os_], np.int64)
    obs_ptr = np.zeros(L + 1, np.int32)
    obs_ptr[1:] = np.cumsum([len(os_) for os_ in obs_of])
    okf = np.asarray(m["obs_kf"])[win_obs].astype(np.int64)
    of = np.asarray(ba["obs_feat"])[win_obs].astype(np.int64)
    pts = np.array(pts, np.int64)
    return dict(P=P, F=F, L=L, nobs=len(win_obs), no_conn=no_conn, dropped=dropped, win_kf=order, win_mp=pts.astype(np.int32),
                win_obs=win_obs.astype(np.int32), obs_ptr=obs_ptr, obs_pose=np.array([index[int(k)] for k in okf], np.int32),
                obs_uvr=np.asarray(ba["kf_uvr"])[okf, of].reshape(-1, 3), obs_oct=np.asarray(ba["kf_oct"])[okf, of].astype(np.int32),
                poses=np.asarray(ba["kf_pose"])[order].reshape(-1, 7), prior=(order[:P] == int(ba.get("kf_first", -1))).astype(np.uint8),
                points=np.asarray(m["mp_pos"])[pts].reshape(-1, 3), assoc=np.asarray(ba["mp_assoc"])[pts].astype(np.int32))


def window_seq(m, ba, kf):
    """one window, following the reference line by line"""
    NMP, NKF, NFK, NOBS = _sizes(m)
    mpv, kfv = _valid(m)
    conn = connections_seq(m, kf)
    ba_local_kf = np.zeros(NKF, bool)  # KeyFrame::ba_local_kf_ == kf_ptr->idx_
    fixed_kf_idx_ba = np.zeros(NKF, bool)
    mp_ba_local_kf = np.zeros(NMP, bool)  # MapPoint::ba_local_kf_ == kf_ptr->idx_
    local_kfs = [kf]  # (:462-463)
    ba_local_kf[kf] = True
    for k in conn["conn_kf"]:  # (:465-471)
        ba_local_kf[k] = True
        if kfv[k]:
            local_kfs.append(int(k))
    local_mappts = []
    for k in local_kfs:  # (:473-489)
        for p in m["kf_mp"][k]:
            p = int(p)
            if p < 0 or p >= NMP:
                continue
            if mpv[p] and not mp_ba_local_kf[p]:
                local_mappts.append(p)
                mp_ba_local_kf[p] = True

    def edges(p):  # the observations that make an edge (:698), malformed ones passed over
        o0, o1 = _range(m, p, NOBS)
        for o in range(o0, o1):
            k, f = int(m["obs_kf"][o]), int(ba["obs_feat"][o])
            if 0 <= k < NKF and 0 <= f < NFK:
                yield o, k
    fixed_kfs = []
    for p in local_mappts:  # (:491-516)
        for o, k in edges(p):
            if not ba_local_kf[k] and not fixed_kf_idx_ba[k]:
                fixed_kf_idx_ba[k] = True
                if kfv[k]:
                    fixed_kfs.append(k)
    pts, obs_of, dropped = [], [], 0
    for p in local_mappts:  # (:639-763)
        os_ = [o for o, k in edges(p) if kfv[k]]
        if not os_ and int(ba["mp_assoc"][p]) < 0:  # no edge: g2o never touches the vertex
            dropped += 1
            continue
        pts.append(p)
        obs_of.append(os_)
    return _pack(m, ba, kf, conn["empty"], local_kfs, fixed_kfs, pts, obs_of, dropped)


def window_vec(m, ba, kf):
    """the same, vectorised"""
    NMP, NKF, NFK, NOBS = _sizes(m)
    mpv, kfv = _valid(m)
    conn = connections_vec(m, kf)
    ck = conn["conn_kf"].astype(np.int64)
    marked = np.zeros(NKF, bool)
    marked[kf] = True
    marked[ck] = True
    free = np.concatenate([[kf], ck[kfv[ck]]]).astype(np.int64)
    held = np.asarray(m["kf_mp"])[free].ravel().astype(np.int64)
    held = held[(held >= 0) & (held < NMP)]
    held = held[mpv[held]]
    _, first = np.unique(held, return_index=True)
    pts = held[np.sort(first)]
    o0, o1 = np.asarray(m["obs_ptr"])[pts].astype(np.int64), np.asarray(m["obs_ptr"])[pts + 1].astype(np.int64)
    ok = (o0 >= 0) & (o1 >= o0) & (o1 <= NOBS)
    n = np.where(ok, o1 - o0, 0)
    flat = np.repeat(o0, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
    owner = np.repeat(np.arange(len(pts)), n)
    k, f = np.asarray(m["obs_kf"])[flat].astype(np.int64), np.asarray(ba["obs_feat"])[flat].astype(np.int64)
    inr = (k >= 0) & (k < NKF) & (f >= 0) & (f < NFK)
    keep = inr & kfv[np.where(inr, k, 0)]
    flat, owner, k = flat[keep], owner[keep], k[keep]
    nobs = np.bincount(owner, minlength=len(pts))
    stay = (nobs > 0) | (np.asarray(ba["mp_assoc"])[pts] >= 0)
    fk = k[~marked[k]]
    _, first = np.unique(fk, return_index=True)
    fixed = fk[np.sort(first)]
    obs_of = np.split(flat, np.cumsum(nobs)[:-1]) if len(pts) else []
    return _pack(m, ba, kf, conn["empty"], free, fixed, pts[stay], [o for o, s in zip(obs_of, stay) if s], int((~stay).sum()))


WINDOW_ARRAYS = ("poses", "prior", "points", "assoc", "obs_ptr", "obs_pose", "obs_uvr", "obs_oct", "win_kf", "win_mp", "win_obs")


def ba_window_build(m, ba, kf_rows, slab, window=window_vec):
    """B windows on the buffers the device works on: slab = dict of the numpy arrays of api.ba_window_slab (the keys of WINDOW_ARRAYS +
    sizes, status) is COPIED, filled as gl_ba_window_build fills it - compact inside the capacities, the entries behind the contents
    left as they were, the true sizes, the truncation bits - and returned with the windows: (slab, [window dict or None])."""
    out = {k: np.array(v) for k, v in slab.items()}
    NKF = m["kf_mp"].shape[0]
    Pcap, PF = out["prior"].shape[1], out["poses"].shape[1]
    Fcap, Lcap, Ocap = PF - Pcap, out["assoc"].shape[1], out["obs_pose"].shape[1]
    wins = []
    for b, kf in enumerate(kf_rows):
        kf = int(kf)
        if kf < 0 or kf >= NKF:
            out["sizes"][b], out["status"][b] = 0, BAD_ROW
            wins.append(None)
            continue
        w = window(m, ba, kf)
        wins.append(w)
        P, F, L, nobs = w["P"], w["F"], w["L"], w["nobs"]
        npf, nl, no = min(P + F, PF), min(L, Lcap), min(nobs, Ocap)
        out["poses"][b, :npf], out["win_kf"][b, :npf] = w["poses"][:npf], w["win_kf"][:npf]
        out["prior"][b, :min(P, Pcap)] = w["prior"][:Pcap]
        for k in ("points", "assoc", "win_mp"):
            out[k][b, :nl] = w[k][:nl]
        out["obs_ptr"][b, :nl] = w["obs_ptr"][:nl]
        if L <= Lcap:
            out["obs_ptr"][b, L] = nobs
        for k in ("obs_pose", "obs_uvr", "obs_oct", "win_obs"):
            out[k][b, :no] = w[k][:no]
        out["sizes"][b] = (P, F, L, nobs)
        out["status"][b] = ((NO_CONN if w["no_conn"] else 0) | (P_TRUNC if P > Pcap else 0) | (F_TRUNC if F > Fcap else 0) | (L_TRUNC if L > Lcap else 0) |
                            (O_TRUNC if nobs > Ocap else 0) | (w["dropped"] << DROPPED_SHIFT))
    return out, wins


# ---- the write-back (:837-853, :898-922)

def twc_of(pose):
    """-(R^T t) of a pose (qx qy qz qw tx ty tz) by the expression gmmloc_hip.h states for gl_ba_window_apply, operation for operation"""
    qx, qy, qz, qw, tx, ty, tz = (np.float64(v) for v in pose)
    n = np.sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw)
    x, y, z, w = qx / n, qy / n, qz / n, qw / n
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return np.array([-((R[0][c] * tx + R[1][c] * ty) + R[2][c] * tz) for c in range(3)])


def ba_window_apply(rows, slab, dropped, erase, iters):
    """rows = dict(kf_pose, kf_twc or None, mp_pos, mp_assoc) is COPIED and updated by a numpy scatter of the slabs after the BA ->
    (rows, [erase_obs per window (ascending CSR positions)])"""
    rows = {k: (None if v is None else np.array(v)) for k, v in rows.items()}
    Pcap, PF = slab["prior"].shape[1], slab["poses"].shape[1]
    Lcap, Ocap = slab["assoc"].shape[1], slab["obs_pose"].shape[1]
    lists = []
    for b in range(slab["sizes"].shape[0]):
        P, F, L, nobs = (int(x) for x in slab["sizes"][b])
        if int(iters[b]) == 0 or P > Pcap or F > PF - Pcap or L > Lcap or nobs > Ocap:
            lists.append(np.zeros(0, np.int32))
            continue
        kf = slab["win_kf"][b, :P]
        rows["kf_pose"][kf] = slab["poses"][b, :P]
        if rows.get("kf_twc") is not None:
            for j in range(P):
                rows["kf_twc"][kf[j]] = twc_of(slab["poses"][b, j])
        mp = slab["win_mp"][b, :L]
        rows["mp_pos"][mp] = slab["points"][b, :L]
        rows["mp_assoc"][mp[dropped[b, :L] != 0]] = -1
        lists.append(np.sort(slab["win_obs"][b, :nobs][erase[b, :nobs] != 0]).astype(np.int32))
    return rows, lists
