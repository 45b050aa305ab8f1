"""What ADDS to the map restated on the sequential object model of tests/map_edit_ref.py - the checker of tests/test_gpu_map_grow.py
(gl_map_add / gl_map_fuse).  Test infrastructure; nothing in the product imports it.

`Model` extends map_edit_ref.Model by subclassing; its methods follow the reference's statements one for one:
  add_observation        MapPoint::addObservation + KeyFrame::addObservation   mappoint.cpp:72-82, keyframe.cpp:190-193
  process_new_key_frame  the loop of Localization::processNewKeyFrame          localization.cpp:424-437
  replace_map_point      Map::replaceMapPoint                                  map.cpp:112-150 (the map part: :113, :116-140)
  fuse_apply             Localization::fuseObservations without the search     localization.cpp:236-241, :299-321
The DECLARED DEVIATION lives in one place, as in map_edit_ref: a dict keeps insertion order, so a gained observation sits behind the
ones the point holds and replace_map_point walks src's observations in that order, where the reference has an unordered_map<pointer>.
`events` counts what a run exercised; tests/test_map_grow_ref.py asserts on it so that no GPU comparison passes vacuously.
map_add / map_fuse are the two calls as the header defines them (lists, skips, capacities) on top of the model."""
import collections

import numpy as np

from tests import map_edit_ref as E

OBS_TRUNCATED, MP_TRUNCATED, REPL_TRUNCATED, ALREADY_TRUNCATED = 1, 2, 4, 8


class Model(E.Model):
    def from_rows(self, m, ba, mp_ref_kf=None):
        super().from_rows(m, ba, mp_ref_kf)
        self.events = collections.Counter()
        self.gained = set()  # (point, key-frame) of every observation gained since from_rows
        self.check_each = False  # check_consistent() after every edit: each candidate of fuse_apply, each triple and walk of map_add

    def new_point(self, ref_kf=-1):
        pt = E.Point()
        pt.row, pt.observations, pt.num_obs, pt.not_valid, pt.was_valid, pt.ref_kf = len(self.points), {}, 0, False, True, int(ref_kf)
        self.points.append(pt)
        return pt

    # ---- the reference's statements
    def check_observation(self, pt, k):
        return k in pt.observations

    def mappoint_add_observation(self, pt, k, f, old_pos=-1):
        """MapPoint::addObservation -> whether it was added"""
        if k in pt.observations:  # (:74-75)
            return False
        pt.observations[k] = f  # (:76)
        pt.num_obs += self.weight(k, f)  # (:78-81)
        self.old_pos[(pt.row, k)] = old_pos
        self.gained.add((pt.row, k))
        return True

    def add_observation(self, pt, k, f):
        """mappt->addObservation(kf, idx); kf->addObservation(mappt, idx) -> whether the point gained the entry"""
        added = self.mappoint_add_observation(pt, k, f)
        self.kfs[k].mappoints[f] = pt.row  # (keyframe.cpp:192)
        return added

    def process_new_key_frame(self, kf):
        """localization.cpp:424-437 -> (candidate_mappts_ as rows, the number of observations added)"""
        candidates, n = [], 0
        for i in range(len(kf.mappoints)):
            pt = self.point_at(kf, i)
            if pt is not None:  # (:426)
                if not pt.not_valid:  # (:427)
                    if not self.check_observation(pt, kf.row):  # (:428)
                        n += self.mappoint_add_observation(pt, kf.row, i)  # (:429)
                    else:
                        candidates.append(pt.row)  # (:433)
        return candidates, n

    def replace_map_point(self, src, tgt):
        """Map::replaceMapPoint"""
        if tgt.row == src.row:  # (:113)
            return
        obs, src.observations = src.observations, {}  # (:119-120)
        src.not_valid = True  # (:121)
        for k, f in obs.items():  # (:127-140)
            pos = self.old_pos.pop((src.row, k))
            self.gained.discard((src.row, k))
            if not self.check_observation(tgt, k):  # (:133)
                self.kfs[k].mappoints[f] = tgt.row  # (:134)
                self.mappoint_add_observation(tgt, k, f, pos)  # (:135)
            else:
                if 0 <= f < self.sizes[2]:
                    self.kfs[k].mappoints[f] = -1  # (:138)
                self.events["nulled"] += 1
                if (tgt.row, k) in self.gained:
                    self.events["chain"] += 1  # only an entry tgt GAINED makes checkObservation true

    def fuse_apply(self, kf, cand_mp, best_idx):
        """localization.cpp:236-241 and :299-321 over the candidates in list order, best_idx in the place of the search
        -> (num_fused, attached, [(src, tgt), ...])"""
        NMP, NKF, NFK, NOBS = self.sizes
        num_fused = attached = 0
        replaced, seen = [], {}
        for c, bi in zip(np.asarray(cand_mp).tolist(), np.asarray(best_idx).tolist()):
            if self.check_each:  # (the map as the candidate before left it)
                self.check_consistent()
            if not 0 <= c < NMP:  # (:236-237 `!mappt`)
                continue
            matched = 0 <= bi < NFK
            pt = self.points[c]
            if pt.not_valid or self.check_observation(pt, kf.row):  # (:239-240)
                if matched and c in seen:
                    self.events["dup_after_" + seen[c]] += 1
                continue
            if not matched:  # (:298)
                continue
            q = kf.mappoints[bi]  # (:299)
            if q >= 0:  # (:300)
                pq = self.points[q] if q < NMP else None
                if pq is not None and not pq.not_valid:  # (:301)
                    if pq.num_obs > pt.num_obs:  # (:303)
                        self.replace_map_point(pt, pq)  # (:306)
                        replaced.append((pt.row, pq.row))
                        self.events["cand_into_q"] += 1
                        seen[c] = "replaced"
                    else:
                        tie = pq.num_obs == pt.num_obs
                        self.replace_map_point(pq, pt)  # (:310)
                        if pq.row != pt.row:
                            replaced.append((pq.row, pt.row))
                            self.events["q_into_cand"] += 1
                            self.events["tie"] += tie
            else:
                attached += self.add_observation(pt, kf.row, bi)  # (:315-316)
                self.events["attach"] += 1
                seen[c] = "attach"
            num_fused += 1  # (:320)
        if self.check_each:
            self.check_consistent()
        return num_fused, attached, replaced

    # ---- objects -> rows
    def to_rows(self):
        """-> dict(mp_valid, kf_valid, kf_mp, obs_ptr, obs_kf, obs_feat, obs_new_pos[, mp_ref_kf]): as map_edit_ref.Model.to_rows, with the
        rows of the new points and obs_new_pos also for the entries that moved to another point"""
        NMP, NKF, NFK, NOBS = self.sizes
        m, ba = self.m, self.ba
        okf, ofeat, ptr, new_pos = [], [], [0], -np.ones(NOBS, np.int32)
        for pt in self.points:
            if not pt.was_valid:
                o0, o1 = E._range(m, pt.row, NOBS)
                new_pos[o0:o1] = len(okf) + np.arange(o1 - o0)
                okf += list(m["obs_kf"][o0:o1])
                ofeat += list(ba["obs_feat"][o0:o1])
            else:
                for k, f in pt.observations.items():
                    if self.old_pos[(pt.row, k)] >= 0:
                        new_pos[self.old_pos[(pt.row, k)]] = len(okf)
                    okf.append(k)
                    ofeat.append(f)
            ptr.append(len(okf))
        rows = dict(mp_valid=np.array([not pt.not_valid for pt in self.points], np.uint8), kf_valid=np.array([not kf.not_valid for kf in self.kfs], np.uint8),
                    kf_mp=np.array([kf.mappoints for kf in self.kfs], np.int32).reshape(NKF, NFK), obs_ptr=np.array(ptr, np.int32),
                    obs_kf=np.array(okf, np.int32), obs_feat=np.array(ofeat, np.int32), obs_new_pos=new_pos)
        if self.ref0 is not None:
            rows["mp_ref_kf"] = np.array([pt.ref_kf for pt in self.points], np.int32)
        return rows

    def check_consistent(self):
        """every observation's slot holds its point, and the weighted count equals the running counter"""
        for pt in self.points:
            if pt.not_valid:
                assert not pt.observations, pt.row
                continue
            w = 0
            for k, f in pt.observations.items():
                assert self.kfs[k].mappoints[f] == pt.row, (pt.row, k, f)
                w += self.weight(k, f)
            assert w == pt.num_obs, (pt.row, w, pt.num_obs)


def _unchanged(m, ba, mp_ref_kf):
    NOBS = len(m["obs_kf"])
    rows = {k: np.array(m[k]) for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")}
    rows.update(obs_feat=np.array(ba["obs_feat"]), obs_new_pos=None)
    if mp_ref_kf is not None:
        rows["mp_ref_kf"] = np.array(mp_ref_kf, np.int32)
    return rows


def map_add(m, ba, mp_ref_kf=None, new_mp=None, new_kf=(), attach=(), walk_kf=(), NMPcap=None, OBScap=None, already_cap=None, model=None):
    """gl_map_add: new_mp dict(pos, assoc, ref_kf) of n rows, new_kf rows, attach [(mp, kf, feat), ...] in list order, walk_kf rows
    -> (rows of Model.to_rows + mp_pos / mp_assoc of the NEW rows + already_mp, result[6]).  Over a capacity: the map as it was,
    obs_new_pos None, the counts and the needed sizes in result."""
    M = Model(m, ba, mp_ref_kf) if model is None else model
    NMP, NKF, NFK, NOBS = M.sizes
    n_new = 0 if new_mp is None else len(new_mp["pos"])
    for i in range(n_new):
        M.new_point(new_mp["ref_kf"][i] if "ref_kf" in new_mp else -1)
    M.sizes = (NMP + n_new, NKF, NFK, NOBS)
    for k in new_kf:
        if 0 <= int(k) < NKF:
            M.kfs[int(k)].not_valid = False
    n_attached = n_skipped = 0
    for p, k, f in attach:
        p, k, f = int(p), int(k), int(f)
        if not (0 <= p < NMP + n_new and 0 <= k < NKF and 0 <= f < NFK) or M.points[p].not_valid or M.kfs[k].not_valid:
            n_skipped += 1
            M.events["skipped"] += 1
            continue
        added = M.add_observation(M.points[p], k, f)
        n_attached += added
        M.events["attach" if added else "dup_triple"] += 1
        if M.check_each:
            M.check_consistent()
    already, walked = [], set()
    for k in walk_kf:
        k = int(k)
        if not 0 <= k < NKF or k in walked or M.kfs[k].not_valid:
            continue
        walked.add(k)
        cands, n = M.process_new_key_frame(M.kfs[k])
        already += cands
        n_attached += n
        if M.check_each:
            M.check_consistent()
    rows = M.to_rows()
    nobs = len(rows["obs_kf"])
    status = (MP_TRUNCATED if NMPcap is not None and NMP + n_new > NMPcap else 0) | (OBS_TRUNCATED if OBScap is not None and nobs > OBScap else 0)
    if already_cap is not None and len(already) > already_cap:
        status |= ALREADY_TRUNCATED
    result = [NMP + n_new, nobs, n_attached, n_skipped, len(already), status]
    if status & (MP_TRUNCATED | OBS_TRUNCATED):
        rows = _unchanged(m, ba, mp_ref_kf)
    elif n_new:
        rows.update(new_pos=np.array(new_mp["pos"], np.float64).reshape(n_new, 3), new_assoc=np.array(new_mp["assoc"], np.int32))
    rows["already_mp"] = np.array(already[:already_cap], np.int32)
    return rows, result


def map_fuse(m, ba, kf, cand_mp, best_idx, OBScap=None, repl_cap=None, model=None):
    """gl_map_fuse -> (rows of Model.to_rows + repl_src / repl_tgt, result[5])"""
    NOBS = len(m["obs_kf"])
    n = len(cand_mp)
    if OBScap is not None and NOBS + n > OBScap:
        rows = _unchanged(m, ba, None)
        rows.update(repl_src=np.zeros(0, np.int32), repl_tgt=np.zeros(0, np.int32))
        return rows, [NOBS + n, 0, 0, 0, OBS_TRUNCATED]
    M = Model(m, ba) if model is None else model
    num_fused, attached, replaced = M.fuse_apply(M.kfs[int(kf)], cand_mp, best_idx)
    rows = M.to_rows()
    cap = len(replaced) if repl_cap is None else repl_cap
    rows.update(repl_src=np.array([s for s, _ in replaced[:cap]], np.int32), repl_tgt=np.array([t for _, t in replaced[:cap]], np.int32))
    return rows, [len(rows["obs_kf"]), num_fused, attached, len(replaced), REPL_TRUNCATED if len(replaced) > cap else 0]


def apply_rows(m, ba, rows, extra=None):
    """the grown map as the dicts the other restatements take (extra: per-point arrays of the new rows to append, by key)"""
    m2 = dict(m, **{k: rows[k] for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")})
    for k, v in (extra or {}).items():
        m2[k] = np.concatenate([m[k], v])
    return m2, dict(ba, obs_feat=rows["obs_feat"])
