"""The oracle of gl_update_map_points: MapPoint::computeDistinctiveDescriptors (mappoint.cpp:126-190) and
MapPoint::updateNormalAndDepth (mappoint.cpp:211-255) restated in numpy, in the reference's loop order.  Test infrastructure
(tests/test_map_point_ref.py, tests/test_gpu_map_points.py, tools/map_points_time.py); nothing in the product imports it.

`refresh_point` is the plain restatement, one point at a time, a Python loop per reference loop.  `update_map_points_ref` gives the
same bytes for a whole map: the descriptor of all points with the same N at once (the same integer distances, sorted rows and first
minimum), the normal as the same left fold over the list positions for all points at once (numpy's element-wise double arithmetic
does not contract); tests/test_map_point_ref.py checks the two against each other.  Inputs: the numpy dicts of
synth.synth_map_points (kf: twc, valid, oct, desc; mp: pos, valid, ref_kf, obs_ptr, obs_kf, obs_feat); outputs: a dict desc,
normal, max_dist, min_dist that is updated in place."""
import math

import numpy as np

POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)
INT_MAX = 2 ** 31 - 1


def scale_factors(scale_factor=1.2):
    """frame::scale_factors (init_config.hpp:67-76): the float recurrence, 8 levels."""
    sf = [np.float32(1.0)]
    for _ in range(7):
        sf.append(np.float32(sf[-1] * np.float32(scale_factor)))
    return np.array(sf, np.float32)


def hamming(a, b):
    """ORBmatcher::DescriptorDistance of two (.., 32) uint8 descriptors."""
    return POP8[np.bitwise_xor(a, b)].sum(-1)


def distinctive_index(descs):
    """The loops of computeDistinctiveDescriptors (:161-185) on the N valid descriptors (N, 32) in list order -> BestIdx."""
    N = len(descs)
    D = [[0] * N for _ in range(N)]
    for i in range(N):
        for j in range(i + 1, N):
            D[i][j] = D[j][i] = int(hamming(descs[i], descs[j]))
    best_median, best_idx = INT_MAX, 0
    for i in range(N):
        median = sorted(D[i])[int(0.5 * (N - 1))]
        if median < best_median:
            best_median, best_idx = median, i
    return best_idx


def _row(kf, mp, p):
    """the observations of point p as [(kf, feat)], or None when the point is to be left untouched (invalid, malformed row)"""
    NKF, NFK = kf["oct"].shape if "oct" in kf else kf["desc"].shape[:2]
    ptr = mp["obs_ptr"]
    NOBS = len(mp["obs_kf"])
    a0, a1 = int(ptr[p]), int(ptr[p + 1])
    if not (0 <= a0 <= a1 <= NOBS):
        return None
    if mp.get("valid") is not None and not mp["valid"][p]:
        return None
    obs = [(int(mp["obs_kf"][a]), int(mp["obs_feat"][a])) for a in range(a0, a1)]
    if any(not (0 <= k < NKF and 0 <= f < NFK) for k, f in obs):
        return None
    return obs


def refresh_point(kf, mp, p, out, what=3, scale_factor=1.2):
    """Both reference functions for point p, one loop at a time."""
    obs = _row(kf, mp, p)
    if not obs:
        return
    kv = kf.get("valid")
    if what & 1:
        descs = [kf["desc"][k, f] for k, f in obs if kv is None or kv[k]]
        if descs:
            out["desc"][p] = descs[distinctive_index(np.array(descs))]
    if what & 2:
        r = int(mp["ref_kf"][p])
        if not (0 <= r < len(kf["twc"])):
            return
        pos = [float(x) for x in mp["pos"][p]]
        normal = [0.0, 0.0, 0.0]
        for k, _ in obs:
            v = [pos[c] - float(kf["twc"][k][c]) for c in range(3)]
            sq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
            if sq > 0.0:  # Eigen 3.3+ normalized(): a zero vector stays zero
                s = math.sqrt(sq)
                v = [v[c] / s for c in range(3)]
            normal = [normal[c] + v[c] for c in range(3)]
        feat = dict(reversed(obs)).get(r, 0)  # the first observation of the ref key-frame; observations[pRefKF] inserts 0 (:245)
        level = int(kf["oct"][r, feat])
        if not 0 <= level < 8:
            return
        sf = scale_factors(scale_factor)
        pc = [pos[c] - float(kf["twc"][r][c]) for c in range(3)]
        dist = np.float32(math.sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]))
        mx = np.float32(dist * sf[level])
        out["max_dist"][p] = mx
        out["min_dist"][p] = np.float32(mx / sf[7])
        out["normal"][p] = [normal[c] / float(len(obs)) for c in range(3)]


def update_map_points_ref(kf, mp, out, what=3, scale_factor=1.2):
    """refresh_point for every point, batched (same bytes)."""
    ptr = mp["obs_ptr"].astype(np.int64)
    NOBS = len(mp["obs_kf"])
    NKF, NFK = kf["oct"].shape if "oct" in kf else kf["desc"].shape[:2]
    ok = (ptr[:-1] >= 0) & (ptr[:-1] < ptr[1:]) & (ptr[1:] <= NOBS)
    if mp.get("valid") is not None:
        ok &= mp["valid"] != 0
    okf = mp["obs_kf"].astype(np.int64)
    off = mp["obs_feat"].astype(np.int64)
    bad_obs = (okf < 0) | (okf >= NKF) | (off < 0) | (off >= NFK)
    cbad = np.concatenate([[0], np.cumsum(bad_obs)])
    ok &= cbad[np.clip(ptr[1:], 0, NOBS)] == cbad[np.clip(ptr[:-1], 0, NOBS)]
    pts = np.nonzero(ok)[0]
    n = (ptr[1:] - ptr[:-1])[pts]
    if what & 1:
        kv = kf.get("valid")
        for p_, N_, idx in _valid_lists(pts, ptr, okf, kv):
            descs = kf["desc"][okf[idx], off[idx]]  # (G, N, 32)
            best = np.empty(len(p_), np.int64)
            step = max(1, (1 << 22) // (N_ * N_ * 32))
            for g0 in range(0, len(p_), step):
                d = descs[g0:g0 + step]
                D = POP8[np.bitwise_xor(d[:, :, None, :], d[:, None, :, :])].sum(-1) if N_ <= 64 else _dist_rows(d)
                med = np.sort(D, axis=-1)[:, :, int(0.5 * (N_ - 1))]
                best[g0:g0 + step] = np.argmin(med, axis=1)  # the first of equal medians
            out["desc"][p_] = descs[np.arange(len(p_)), best]
    if what & 2:
        r = mp["ref_kf"].astype(np.int64)[pts]
        inr = (r >= 0) & (r < NKF)
        pts, n, r = pts[inr], n[inr], r[inr]
        pos = mp["pos"][pts]
        px, py, pz = pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy()
        nx, ny, nz = np.zeros(len(pts)), np.zeros(len(pts)), np.zeros(len(pts))
        feat = np.zeros(len(pts), np.int64)
        found = np.zeros(len(pts), bool)
        twc = kf["twc"]
        for j in range(int(n.max()) if len(n) else 0):  # list position j of every point that has one: the same left fold
            act = np.nonzero(n > j)[0]
            a = ptr[pts[act]] + j
            k = okf[a]
            hit = ~found[act] & (k == r[act])
            feat[act[hit]] = off[a[hit]]
            found[act[hit]] = True
            vx, vy, vz = px[act] - twc[k, 0], py[act] - twc[k, 1], pz[act] - twc[k, 2]
            sq = vx * vx + vy * vy + vz * vz
            s = np.sqrt(np.where(sq > 0.0, sq, 1.0))
            nz_ = sq > 0.0
            vx, vy, vz = np.where(nz_, vx / s, vx), np.where(nz_, vy / s, vy), np.where(nz_, vz / s, vz)
            nx[act], ny[act], nz[act] = nx[act] + vx, ny[act] + vy, nz[act] + vz
        level = kf["oct"][r, feat].astype(np.int64)
        lv = (level >= 0) & (level < 8)
        sf = scale_factors(scale_factor)
        cx, cy, cz = px - twc[r, 0], py - twc[r, 1], pz - twc[r, 2]
        dist = np.sqrt(cx * cx + cy * cy + cz * cz).astype(np.float32)
        mx = (dist * sf[np.clip(level, 0, 7)]).astype(np.float32)
        q = pts[lv]
        out["max_dist"][q] = mx[lv]
        out["min_dist"][q] = (mx / sf[7]).astype(np.float32)[lv]
        nd = n.astype(np.float64)
        out["normal"][q] = np.stack([nx / nd, ny / nd, nz / nd], 1)[lv]
    return out


def _valid_lists(pts, ptr, okf, kv):
    """per N: (points, N, (G, N) observation indices of their valid observations in list order)"""
    lists = {}
    for p in pts:
        a = np.arange(ptr[p], ptr[p + 1])
        if kv is not None:
            a = a[kv[okf[a]] != 0]
        if len(a):
            lists.setdefault(len(a), []).append((p, a))
    for N_, items in sorted(lists.items()):
        yield np.array([p for p, _ in items]), N_, np.stack([a for _, a in items])


def _dist_rows(d):
    """the distance matrices of (G, N, 32) descriptors row block by row block (large N)"""
    G, N_, _ = d.shape
    D = np.empty((G, N_, N_), np.int32)
    for i0 in range(0, N_, 64):
        D[:, i0:i0 + 64] = POP8[np.bitwise_xor(d[:, i0:i0 + 64, None, :], d[:, None, :, :])].sum(-1)
    return D
