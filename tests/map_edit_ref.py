"""The removals and the key-frame culling of the reference restated as a small SEQUENTIAL object model on the flat map arrays of
gl_cull_keyframes / gl_map_remove - the checker of tests/test_gpu_map_edit.py.  Test infrastructure; nothing in the product imports it.

`Model` keeps what the reference keeps: a point with its observations (a dict key-frame row -> feature index, in CSR order) and its
counter num_obs_, a key-frame with mappoints_ and not_valid_.  Its methods follow the reference's statements one for one, in the order
they are called:
  remove_observation   MapPoint::removeObservation      mappoint.cpp:94-118  (the weights of addObservation :72-82)
  remove_map_point     Map::removeMapPoint              map.cpp:40-58
  remove_key_frame     Map::removeKeyFrame              map.cpp:60-110 (the map part: :63-64, :70-76, :86)
  ba_erase             the erase loop of the local BA   localization_opt.cpp:884-894 (KeyFrame::removeObservation keyframe.cpp:200-205)
  remove_key_frames    Localization::removeKeyFrames    localization.cpp:334-399
The DECLARED DEVIATION lives in one place: a dict keeps insertion order, so observations_.begin() (mappoint.cpp:109) is the first
surviving CSR entry, where the reference has the first bucket of an unordered_map<pointer>.
What the rows can hold and the reference's containers cannot is decided as gmmloc_hip.h decides it: a point or key-frame that is
invalid on entry, a duplicate, a row outside its table change nothing.  A point that is invalid on entry has NO observations in the
model (Map::removeMapPoint cleared them, :47); the CSR entries its rows may still hold are passed through by to_rows untouched.
`cull_by_state` says the culling loop a second way - what candidate j reads is a function of the set C culled before it - directly on
the arrays; it is also the definition on a malformed map, where the CSR decides what a key-frame observes."""
import numpy as np

JUDGED, FIRST, BAD_ROW, INVALID, DUPLICATE = 0, 1, 2, 3, 4
FIRST_REFUSED, DEAD_TRUNCATED = 1, 2
TH_OBS = 3  # localization.cpp:349-350


def _sizes(m):
    return len(m["obs_ptr"]) - 1, m["kf_mp"].shape[0], m["kf_mp"].shape[1], len(m["obs_kf"])


def _range(m, p, NOBS):
    o0, o1 = int(m["obs_ptr"][p]), int(m["obs_ptr"][p + 1])
    return (o0, o1) if 0 <= o0 <= o1 <= NOBS else (0, 0)


class Point:
    __slots__ = ("row", "observations", "num_obs", "not_valid", "ref_kf", "was_valid")


class KeyFrame:
    __slots__ = ("row", "mappoints", "not_valid", "was_valid")


class Model:
    def __init__(self, m, ba, mp_ref_kf=None):
        self.from_rows(m, ba, mp_ref_kf)

    # ---- rows -> objects
    def from_rows(self, m, ba, mp_ref_kf=None):
        NMP, NKF, NFK, NOBS = self.sizes = _sizes(m)
        self.m, self.ba = m, ba
        self.kf_first = int(ba.get("kf_first", -1))
        self.mono = np.asarray(ba["kf_uvr"])[:, :, 2] < 0  # (u_right >= 0: a stereo observation, mappoint.cpp:78)
        self.oct = np.asarray(ba["kf_oct"])
        self.ref0 = None if mp_ref_kf is None else np.array(mp_ref_kf, np.int32)
        obs_kf, obs_feat = np.asarray(m["obs_kf"]).tolist(), np.asarray(ba["obs_feat"]).tolist()
        mpv, kfv = np.asarray(m["mp_valid"]) != 0, np.asarray(m["kf_valid"]) != 0
        self.old_pos = {}  # (point, key-frame) -> CSR position on entry
        self.entry = [None] * NOBS  # CSR position -> (key-frame, point)
        self.points, self.kfs = [], []
        self.dead = []
        for p in range(NMP):
            pt = Point()
            pt.row, pt.observations, pt.num_obs, pt.not_valid, pt.was_valid = p, {}, 0, not mpv[p], bool(mpv[p])
            pt.ref_kf = -1 if mp_ref_kf is None else int(mp_ref_kf[p])
            o0, o1 = _range(m, p, NOBS)
            for o in range(o0, o1):
                k, f = obs_kf[o], obs_feat[o]
                if not 0 <= k < NKF:
                    continue
                self.entry[o] = (k, p)
                if pt.not_valid or k in pt.observations:
                    continue
                pt.observations[k] = f
                pt.num_obs += self.weight(k, f)
                self.old_pos[(p, k)] = o
            self.points.append(pt)
        kf_mp = np.asarray(m["kf_mp"])
        for k in range(NKF):
            kf = KeyFrame()
            kf.row, kf.mappoints, kf.not_valid, kf.was_valid = k, kf_mp[k].tolist(), not kfv[k], bool(kfv[k])
            self.kfs.append(kf)

    def weight(self, k, f):
        if not 0 <= f < self.sizes[2]:
            return 0
        return 1 if self.mono[k, f] else 2

    def point_at(self, kf, i):
        p = kf.mappoints[i]
        return self.points[p] if 0 <= p < self.sizes[0] else None

    # ---- the reference's statements
    def remove_observation(self, pt, k):
        """MapPoint::removeObservation -> bBad"""
        bad = False
        if k in pt.observations:  # (:99)
            f = pt.observations[k]
            pt.num_obs -= self.weight(k, f)  # (:101-104)
            del pt.observations[k]  # (:106)
            if pt.num_obs > 0 and pt.ref_kf == k and pt.observations:  # (:108-110)
                pt.ref_kf = next(iter(pt.observations))
            if pt.num_obs <= 2:  # (:112-113)
                bad = True
        return bad

    def remove_map_point(self, pt):
        """Map::removeMapPoint"""
        if pt.not_valid:
            return
        pt.not_valid = True  # (:45)
        observations, pt.observations = pt.observations, {}  # (:46-47)
        for k, f in observations.items():  # (:49-52)
            if 0 <= f < self.sizes[2]:
                self.kfs[k].mappoints[f] = -1
        self.dead.append(pt.row)

    def remove_key_frame(self, kf):
        """Map::removeKeyFrame -> False where it is refused (:63-64)"""
        if kf.row == self.kf_first:
            return False
        if kf.not_valid:
            return True
        for i in range(len(kf.mappoints)):  # (:70-76: the key-frame's own mappoints_ are never nulled here)
            pt = self.point_at(kf, i)
            if pt is not None and self.remove_observation(pt, kf.row):
                self.remove_map_point(pt)
        kf.not_valid = True  # (:86)
        return True

    def ba_erase(self, positions):
        """localization_opt.cpp:884-894 on vToErase given as CSR positions of the map on entry"""
        for o in positions:
            o = int(o)
            if not 0 <= o < self.sizes[3] or self.entry[o] is None:
                continue
            k, p = self.entry[o]
            pt = self.points[p]
            f = pt.observations.get(k, -1)  # KeyFrame::removeObservation(MapPoint*): getIndexInKeyFrame
            if 0 <= f < self.sizes[2]:
                self.kfs[k].mappoints[f] = -1
            if self.remove_observation(pt, k):
                self.remove_map_point(pt)

    def remove_key_frames(self, cands, kf_depth, th_depth):
        """Localization::removeKeyFrames over the list `cands` -> dict(cull, num_mps, num_redundant, status, cull_rows)"""
        NMP, NKF, NFK, NOBS = self.sizes
        th = np.float32(th_depth)
        n = len(cands)
        out = dict(cull=np.zeros(n, np.uint8), num_mps=np.zeros(n, np.int32), num_redundant=np.zeros(n, np.int32), status=np.zeros(n, np.int32), cull_rows=[])
        seen = set()
        for j, row in enumerate(cands):
            row = int(row)
            if not 0 <= row < NKF:
                out["status"][j] = BAD_ROW
                continue
            if row in seen:
                out["status"][j] = DUPLICATE
                continue
            seen.add(row)
            kf = self.kfs[row]
            if row == self.kf_first:  # (:344)
                out["status"][j] = FIRST
                continue
            if kf.not_valid:
                out["status"][j] = INVALID
                continue
            num_redundant = num_mps = 0
            depth = kf_depth[row]
            for i in range(NFK):
                pt = self.point_at(kf, i)
                if pt is None or pt.not_valid:  # (:356)
                    continue
                if depth[i] > th or depth[i] < 0:  # (:358-362)
                    continue
                num_mps += 1
                if pt.num_obs > TH_OBS:  # (:366)
                    scale = int(self.oct[row, i])
                    num_obs = 0
                    for k, f in pt.observations.items():  # (:372-386)
                        if k == row or not 0 <= f < NFK:
                            continue
                        if self.oct[k, f] <= scale + 1:
                            num_obs += 1
                    if num_obs >= TH_OBS:
                        num_redundant += 1
            out["num_mps"][j], out["num_redundant"][j] = num_mps, num_redundant
            if float(num_redundant) > 0.9 * float(num_mps):  # (:394-396)
                out["cull"][j] = 1
                out["cull_rows"].append(row)
                self.remove_key_frame(kf)
        out["cull_rows"] = np.array(out["cull_rows"], np.int32)
        return out

    # ---- objects -> rows
    def to_rows(self):
        """-> dict(mp_valid, kf_valid, kf_mp, obs_ptr, obs_kf, obs_feat, obs_new_pos, dead_mp[, mp_ref_kf]).  The entries of a point that
        was invalid on entry are passed through; mp_ref_kf of a point that died is what it was on entry."""
        NMP, NKF, NFK, NOBS = self.sizes
        m, ba = self.m, self.ba
        okf, ofeat, ptr, new_pos = [], [], [0], -np.ones(NOBS, np.int32)
        for pt in self.points:
            if not pt.was_valid:
                o0, o1 = _range(m, pt.row, NOBS)
                new_pos[o0:o1] = len(okf) + np.arange(o1 - o0)
                okf += list(m["obs_kf"][o0:o1])
                ofeat += list(ba["obs_feat"][o0:o1])
            else:
                for k, f in pt.observations.items():
                    new_pos[self.old_pos[(pt.row, k)]] = len(okf)
                    okf.append(k)
                    ofeat.append(f)
            ptr.append(len(okf))
        rows = dict(mp_valid=np.array([not pt.not_valid for pt in self.points], np.uint8), kf_valid=np.array([not kf.not_valid for kf in self.kfs], np.uint8),
                    kf_mp=np.array([kf.mappoints for kf in self.kfs], np.int32).reshape(NKF, NFK), obs_ptr=np.array(ptr, np.int32),
                    obs_kf=np.array(okf, np.int32), obs_feat=np.array(ofeat, np.int32), obs_new_pos=new_pos, dead_mp=np.array(sorted(self.dead), np.int32))
        if self.ref0 is not None:
            rows["mp_ref_kf"] = np.array([self.ref0[pt.row] if pt.not_valid else pt.ref_kf for pt in self.points], np.int32)
        return rows


def map_remove(m, ba, rm_mp=(), erase_obs=(), rm_kf=(), mp_ref_kf=None):
    """what gl_map_remove applies: the points, then the observations, then the key-frames in list order -> (rows of Model.to_rows, status)"""
    M = Model(m, ba, mp_ref_kf)
    NMP, NKF = M.sizes[:2]
    status = 0
    for p in rm_mp:
        if 0 <= int(p) < NMP:
            M.remove_map_point(M.points[int(p)])
    M.ba_erase(erase_obs)
    for k in rm_kf:
        if 0 <= int(k) < NKF and not M.kfs[int(k)].not_valid:
            if not M.remove_key_frame(M.kfs[int(k)]):
                status |= FIRST_REFUSED
    return M.to_rows(), status


def apply_rows(m, ba, rows):
    """the edited map as the dicts the other restatements take"""
    m2 = dict(m, **{k: rows[k] for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")})
    return m2, dict(ba, obs_feat=rows["obs_feat"])


# ---- the culling loop once more: the state as a function of the set C

def cull_by_state(m, ba, cands, kf_depth, th_depth):
    """the verdicts of removeKeyFrames with NOTHING removed: an observation by a key-frame in C does not exist; a point is dead iff a
    key-frame in C observes it and its weighted count over the observers outside C is <= 2.  Vectorised per candidate; malformed input
    is skipped as gmmloc_hip.h says."""
    NMP, NKF, NFK, NOBS = _sizes(m)
    mpv, kfv = np.asarray(m["mp_valid"]) != 0, np.asarray(m["kf_valid"]) != 0
    obs_kf, obs_feat = np.asarray(m["obs_kf"]).astype(np.int64), np.asarray(ba["obs_feat"]).astype(np.int64)
    kin = (obs_kf >= 0) & (obs_kf < NKF)
    fin = kin & (obs_feat >= 0) & (obs_feat < NFK)
    kk, ff = np.where(fin, obs_kf, 0), np.where(fin, obs_feat, 0)
    wgt = np.where(fin, np.where(np.asarray(ba["kf_uvr"])[kk, ff, 2] >= 0, 2, 1), 0)
    octo = np.asarray(ba["kf_oct"])[kk, ff]
    ptr = np.asarray(m["obs_ptr"]).astype(np.int64)
    okr = (ptr[:-1] >= 0) & (ptr[1:] >= ptr[:-1]) & (ptr[1:] <= NOBS)
    th = np.float32(th_depth)
    inC = np.zeros(NKF, bool)
    first = int(ba.get("kf_first", -1))
    n = len(cands)
    out = dict(cull=np.zeros(n, np.uint8), num_mps=np.zeros(n, np.int32), num_redundant=np.zeros(n, np.int32), status=np.zeros(n, np.int32), cull_rows=[])
    seen = set()
    for j, row in enumerate(cands):
        row = int(row)
        st = BAD_ROW if not 0 <= row < NKF else DUPLICATE if row in seen else FIRST if row == first else INVALID if not kfv[row] else JUDGED
        if st not in (BAD_ROW, DUPLICATE):
            seen.add(row)
        out["status"][j] = st
        if st != JUDGED:
            continue
        held = np.asarray(m["kf_mp"][row]).astype(np.int64)
        slot = np.nonzero((held >= 0) & (held < NMP))[0]
        slot = slot[mpv[held[slot]]]
        p = held[slot]
        cnt = np.where(okr[p], ptr[p + 1] - ptr[p], 0)
        flat = np.repeat(np.where(okr[p], ptr[p], 0), cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        own = np.repeat(np.arange(len(p)), cnt)
        gone = kin[flat] & inC[np.where(kin[flat], obs_kf[flat], 0)]
        live = kin[flat] & ~gone
        w = np.bincount(own, (wgt[flat] * live), len(p))
        byC = np.bincount(own, gone, len(p)) > 0
        near = np.bincount(own, live & fin[flat] & (obs_kf[flat] != row) & (octo[flat] <= np.repeat(np.asarray(ba["kf_oct"])[row, slot], cnt) + 1), len(p))
        d = kf_depth[row, slot]
        counted = ~(byC & (w <= 2)) & ~((d > th) | (d < 0))
        nm, nr = int(counted.sum()), int((counted & (w > 3) & (near >= 3)).sum())
        out["num_mps"][j], out["num_redundant"][j] = nm, nr
        if float(nr) > 0.9 * float(nm):
            out["cull"][j] = 1
            out["cull_rows"].append(row)
            inC[row] = True
    out["cull_rows"] = np.array(out["cull_rows"], np.int32)
    return out


def cull_keyframes(m, ba, cand, n_cand, kf_depth, th_depth, out, judge=None):
    """B lists on the buffers the device works on: out = dict(cull, num_mps, num_redundant, cand_status, cull_rows (B,Ccap), n_cull (B,)) is
    COPIED, filled as gl_cull_keyframes fills it and returned.  judge(list) -> the dict of Model.remove_key_frames / cull_by_state
    (default: the sequential model, on a fresh model per list)."""
    if judge is None:
        judge = lambda lst: Model(m, ba).remove_key_frames(lst, kf_depth, th_depth)
    out = {k: np.array(v) for k, v in out.items()}
    Ccap = cand.shape[1]
    done = {}
    for b in range(cand.shape[0]):
        n = min(max(int(n_cand[b]), 0), Ccap)
        key = cand[b, :n].tobytes()
        if key not in done:
            done[key] = judge(cand[b, :n])
        r = done[key]
        out["cull"][b, :n], out["num_mps"][b, :n], out["num_redundant"][b, :n], out["cand_status"][b, :n] = r["cull"], r["num_mps"], r["num_redundant"], r["status"]
        out["cull_rows"][b, :len(r["cull_rows"])] = r["cull_rows"]
        out["n_cull"][b] = len(r["cull_rows"])
    return out
