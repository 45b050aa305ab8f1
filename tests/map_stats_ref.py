"""num_visible_ / num_found_ / ref_idx_ and Localization::removeMapPoints restated on the sequential object model of
tests/map_grow_ref.py - the checker of tests/test_gpu_map_stats.py (gl_map_stats_track, gl_map_stats_new_points, gl_map_cand_append,
gl_map_stats_merge, gl_cull_map_points).  Test infrastructure; nothing in the product imports it.

`Model` extends map_grow_ref.Model by subclassing.  It keeps the three fields per point (lists indexed by the point's row: the points
of map_edit_ref are slotted objects) and candidate_mappts_ as a Python list of rows; its methods follow the reference's statements one
for one:
  new_point                   the key-frame constructor of MapPoint        mappoint.cpp:18-19 (ref_idx_ default: mappoint.h:86)
  search_local_points_stats   Tracking::searchLocalPoints, the counters    tracking.cpp:213-225, :233-254
  track_local_map_stats       Tracking::trackLocalMap, the counters        tracking.cpp:279-292
  replace_map_point           Map::replaceMapPoint with its counters       map.cpp:112-150 (:124-125, :142-143)
  remove_map_points           Localization::removeMapPoints                localization.cpp:127-152, with REAL list erasure and real
                                                                            Map::removeMapPoint calls
`events` (map_grow_ref) counts every branch that ran; tests/test_map_stats_ref.py asserts on it so that no comparison passes vacuously.
judge_snapshot says removeMapPoints the second way - one pass over a snapshot plus a first-occurrence rule, what the kernel does - and
tests/test_map_stats_ref.py shows the two equal.  Counters wrap like fetch_add on atomic_int; ratios are np.float32 divisions."""
import numpy as np

from tests import map_grow_ref as G

KEPT, INVALID, RATIO, YOUNG_FEW, AGED, BAD_ROW = 0, 1, 2, 3, 4, 5
MP_TRUNCATED, CAND_TRUNCATED, STATUS_BAD_ROW = 1, 2, 4
TEMPORAL = -2  # a feature that holds a TEMPORAL point (createTemporalPoints): non-null, no row, no counter
CN_TH_OBS = 3  # localization.cpp:131


def wrap(x):
    """32-bit two's-complement wrap-around"""
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def found_ratio(found, visible):
    """static_cast<float>(num_found_) / num_visible_ (localization.cpp:135-136): two int -> float conversions, one float division"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(found) / np.float32(visible)


class Model(G.Model):
    def from_rows(self, m, ba, mp_ref_kf=None):
        super().from_rows(m, ba, mp_ref_kf)
        n = len(self.points)
        self.num_visible, self.num_found, self.ref_idx = [1] * n, [1] * n, [-1] * n
        self.kf_idx = None  # idx_ per key-frame row; None: the row
        self.cand = []  # candidate_mappts_

    def set_stats(self, visible, found, ref_idx, kf_idx=None, cand=()):
        n = len(self.points)
        self.num_visible, self.num_found, self.ref_idx = ([int(v) for v in np.asarray(a)[:n]] for a in (visible, found, ref_idx))
        self.kf_idx = None if kf_idx is None else [int(v) for v in kf_idx]
        self.cand = [int(v) for v in cand]
        return self

    def idx_of(self, k):
        if not 0 <= k < self.sizes[1]:
            return -1  # (mappoint.h:86)
        return k if self.kf_idx is None else self.kf_idx[k]

    def new_point(self, ref_kf=-1):
        pt = super().new_point(ref_kf)
        self.num_visible.append(1)  # (mappoint.cpp:19)
        self.num_found.append(1)
        self.ref_idx.append(self.idx_of(int(ref_kf)))  # (mappoint.cpp:18)
        return pt

    def _point(self, row):
        return self.points[row] if 0 <= row < len(self.points) else None

    # ---- the reference's statements
    def search_local_points_stats(self, frame_mps, local_mps, in_view, seen=()):
        """tracking.cpp:213-254.  frame_mps: per feature the row it holds (-1 null, TEMPORAL), IN/OUT; local_mps: local_mappoints_ as
        rows; in_view[s]: project3 && checkScaleAndVisible of slot s; seen: rows whose last_visible_idx_ is this frame's already (the
        points the frame dropped as outliers, tracking.cpp:367)."""
        visible_now = set(seen)
        for i, row in enumerate(frame_mps):  # (:213-216)
            pt = self._point(row)
            if row == TEMPORAL:
                self.events["held_temporal"] += 1
            if pt is not None:  # (:218)
                if pt.not_valid:  # (:219)
                    frame_mps[i] = -1  # (:220)
                    self.events["held_invalid"] += 1
                else:
                    self.num_visible[row] = wrap(self.num_visible[row] + 1)  # (:222)
                    self.events["held_twice" if row in visible_now else "held"] += 1
                    visible_now.add(row)  # (:223)
        for s, row in enumerate(local_mps):  # (:237)
            pt = self._point(row)
            if pt is None:
                continue
            if row in visible_now:  # (:241)
                continue
            if pt.not_valid:  # (:243)
                continue
            if in_view[s]:  # (:248-252)
                self.num_visible[row] = wrap(self.num_visible[row] + 1)  # (:256)
                self.events["in_view"] += 1

    def track_local_map_stats(self, frame_mps, is_outlier):
        """tracking.cpp:279-292.  frame_mps IN/OUT: an outlier loses its map point."""
        for i, row in enumerate(frame_mps):  # (:279)
            if row == -1:  # (:280)
                continue
            if not is_outlier[i]:  # (:282)
                if self._point(row) is not None:
                    self.num_found[row] = wrap(self.num_found[row] + 1)  # (:283)
                    self.events["found"] += 1
            else:
                frame_mps[i] = -1  # (:289)
                self.events["outlier"] += 1

    def replace_map_point(self, src, tgt):
        """Map::replaceMapPoint with its counters"""
        if tgt.row == src.row:  # (:113)
            self.events["replace_self"] += 1
            return
        nvisible, nfound = self.num_visible[src.row], self.num_found[src.row]  # (:124-125)
        super().replace_map_point(src, tgt)
        self.num_visible[tgt.row] = wrap(self.num_visible[tgt.row] + nvisible)  # (:142)
        self.num_found[tgt.row] = wrap(self.num_found[tgt.row] + nfound)  # (:143)
        self.events["replace"] += 1

    def remove_map_points(self, kf_row):
        """Localization::removeMapPoints -> (verdict per OLD entry, the rows given to Map::removeMapPoint in order).  self.cand is the
        list afterwards.  DECLARED: an entry outside [0, NMP) is erased (BAD_ROW); the reference's list holds no such entry."""
        curr_idx = self.idx_of(int(kf_row))  # (:129)
        verdict, removed = [], []
        lit = 0
        while lit != len(self.cand):  # (:133)
            row = self.cand[lit]
            pt = self._point(row)
            if pt is None:
                verdict.append(BAD_ROW)
                del self.cand[lit]
                self.events["bad_row"] += 1
                continue
            ratio = found_ratio(self.num_found[row], self.num_visible[row])  # (:135-136)
            if pt.not_valid:  # (:137)
                verdict.append(INVALID)
                del self.cand[lit]  # (:138)
                self.events["invalid_again" if row in removed else "invalid"] += 1
            elif ratio < np.float32(0.25):  # (:139)
                self.remove_map_point(pt)  # (:140)
                removed.append(row)
                verdict.append(RATIO)
                del self.cand[lit]  # (:141)
                self.events["ratio"] += 1
            elif curr_idx - self.ref_idx[row] >= 2 and pt.num_obs <= CN_TH_OBS:  # (:142-143)
                self.remove_map_point(pt)  # (:144)
                removed.append(row)
                verdict.append(YOUNG_FEW)
                del self.cand[lit]  # (:145)
                self.events["young_few"] += 1
            elif curr_idx - self.ref_idx[row] >= 3:  # (:146)
                verdict.append(AGED)
                del self.cand[lit]  # (:147)
                self.events["aged"] += 1
            else:
                verdict.append(KEPT)
                lit += 1  # (:149)
                self.events["kept"] += 1
                if not ratio == ratio or np.isinf(ratio):
                    self.events["kept_nan_inf"] += 1
        return verdict, removed

    # ---- the same as one pass over a snapshot (what gl_cull_map_points does)
    def judge_row(self, row, curr_idx):
        """the branches of removeMapPoints for ONE row on the state as it is, nothing changed"""
        pt = self.points[row]
        if pt.not_valid:
            return INVALID
        if found_ratio(self.num_found[row], self.num_visible[row]) < np.float32(0.25):
            return RATIO
        age = curr_idx - self.ref_idx[row]
        if age >= 2 and pt.num_obs <= CN_TH_OBS:
            return YOUNG_FEW
        return AGED if age >= 3 else KEPT

    def judge_snapshot(self, kf_row, cand=None):
        """-> (verdict per entry, the kept list, rm_mp): every entry judged on the UNCHANGED state; a later occurrence of a row whose
        first occurrence removes it is INVALID"""
        cand = self.cand if cand is None else cand
        curr_idx = self.idx_of(int(kf_row))
        first, verdict = {}, []
        for i, row in enumerate(cand):
            if not 0 <= row < len(self.points):
                verdict.append(BAD_ROW)
                continue
            v = self.judge_row(row, curr_idx)
            if v in (RATIO, YOUNG_FEW) and first.setdefault(row, i) != i:
                v = INVALID
            first.setdefault(row, i)
            verdict.append(v)
        kept = [row for row, v in zip(cand, verdict) if v == KEPT]
        rm = [row for row, v in zip(cand, verdict) if v in (RATIO, YOUNG_FEW)]
        return verdict, kept, rm

    def stats_arrays(self, NMPcap=None):
        """-> (visible, found, ref_idx) int32, padded with (0, 0, -1) to NMPcap rows"""
        n = len(self.points)
        cap = n if NMPcap is None else NMPcap
        out = []
        for a, fill in ((self.num_visible, 0), (self.num_found, 0), (self.ref_idx, -1)):
            v = np.full(cap, fill, np.int32)
            v[:n] = a
            out.append(v)
        return out


# ---- the five calls as the header defines them, on plain arrays (what the device is compared with where no map is involved)

def track(visible, found, NMP, feat_mp, match_local, outlier, inview, local_mp, n_local_mp, counts2=None):
    """gl_map_stats_track stated directly: -> (visible, found) after B frames"""
    vis, fnd = np.array(visible, np.int64), np.array(found, np.int64)
    B, NF = feat_mp.shape
    NPcap = local_mp.shape[1]
    for b in range(B):
        if counts2 is not None and counts2[b, 3] == 2:
            continue
        for i in range(NF):
            h = int(feat_mp[b, i])
            if 0 <= h < NMP:
                vis[h] += 1
            if outlier[b, i]:
                continue
            j = int(match_local[b, i])
            r = (int(local_mp[b, j]) if j < NPcap else -1) if j >= 0 else h
            if 0 <= r < NMP:
                fnd[r] += 1
        for s in range(min(max(int(n_local_mp[b]), 0), NPcap)):
            r = int(local_mp[b, s])
            if inview[b, s] and 0 <= r < NMP:
                vis[r] += 1
    w = lambda a: ((a + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)
    return w(vis), w(fnd)


def model_track(M, feat_mp, match_local, outlier, inview, local_mp, n_local_mp, counts2=None):
    """the chain's outputs fed to the model's statements, frame by frame: feat_mp is what the frame holds on entry to
    searchLocalPoints, match_local what searchByProjection added, outlier what optimizeCurrentPose left"""
    B, NF = feat_mp.shape
    NPcap = local_mp.shape[1]
    for b in range(B):
        if counts2 is not None and counts2[b, 3] == 2:  # (tracking.cpp:62-72)
            M.events["lost"] += 1
            continue
        n = min(max(int(n_local_mp[b]), 0), NPcap)
        frame = [int(v) for v in feat_mp[b]]
        local = [int(v) for v in local_mp[b, :n]]
        M.search_local_points_stats(frame, local, inview[b])
        for i in range(NF):  # (searchByProjection: a free feature takes its match)
            j = int(match_local[b, i])
            if 0 <= j < NPcap:
                frame[i] = int(local_mp[b, j])
                M.events["matched_local"] += 1
        M.track_local_map_stats(frame, outlier[b])


def merge(visible, found, NMP, src, tgt):
    """gl_map_stats_merge stated directly, in step order"""
    vis, fnd = [int(v) for v in visible], [int(v) for v in found]
    for s, t in zip(np.asarray(src).tolist(), np.asarray(tgt).tolist()):
        if s == t or not (0 <= s < NMP and 0 <= t < NMP):
            continue
        vis[t] = wrap(vis[t] + vis[s])
        fnd[t] = wrap(fnd[t] + fnd[s])
    return np.array(vis, np.int32), np.array(fnd, np.int32)


def cull_arrays(m, ba, visible, found, ref_idx, kf_idx, kf_row, cand):
    """gl_cull_map_points stated directly on the arrays - also the definition on a malformed map: the weight from the CSR and kf_uvr
    (an entry outside the tables weighs 0, a range outside [0, NOBS] has no entry)
    -> (verdict per entry, the list afterwards, rm_mp, result[4])"""
    NMP, NKF, NFK, NOBS = len(m["mp_valid"]), m["kf_mp"].shape[0], m["kf_mp"].shape[1], len(m["obs_kf"])
    curr = int(kf_row) if kf_idx is None else int(kf_idx[kf_row])
    uvr = np.asarray(ba["kf_uvr"])

    def judge(p):
        if not m["mp_valid"][p]:
            return INVALID
        if found_ratio(int(found[p]), int(visible[p])) < np.float32(0.25):
            return RATIO
        age = curr - int(ref_idx[p])
        o0, o1 = int(m["obs_ptr"][p]), int(m["obs_ptr"][p + 1])
        w = 0
        if 0 <= o0 <= o1 <= NOBS:
            for o in range(o0, o1):
                k, f = int(m["obs_kf"][o]), int(ba["obs_feat"][o])
                if 0 <= k < NKF and 0 <= f < NFK:
                    w += 2 if uvr[k, f, 2] >= 0 else 1
        if age >= 2 and w <= CN_TH_OBS:
            return YOUNG_FEW
        return AGED if age >= 3 else KEPT

    verdict, seen, status = [], set(), 0
    for p in np.asarray(cand).tolist():
        if not 0 <= p < NMP:
            verdict.append(BAD_ROW)
            status |= STATUS_BAD_ROW
            continue
        v = judge(p)
        if v in (RATIO, YOUNG_FEW) and p in seen:
            v = INVALID
        seen.add(p)
        verdict.append(v)
    kept = [p for p, v in zip(np.asarray(cand).tolist(), verdict) if v == KEPT]
    rm = [p for p, v in zip(np.asarray(cand).tolist(), verdict) if v in (RATIO, YOUNG_FEW)]
    return verdict, kept, rm, [len(kept), len(rm), len(verdict) - len(kept) - len(rm), status]
