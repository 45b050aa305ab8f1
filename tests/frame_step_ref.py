"""The stretch between two tracked frames on a small sequential object model - the checker of tests/test_gpu_frame_step.py and
tests/test_frame_step_cases.py (gl_track_frame_end, gl_map_note_replaced, gl_track_frame_next).  Test infrastructure; nothing in the
product imports it, and it imports nothing of the device glue.

Objects as in the reference: a `Frame` with mappoints_ (MapPoint objects or None), is_outlier_, the features' depths, a pose and T_c_r;
`MapPoint`s with a weighted num_obs_ (countObservations), not_valid_ and ptr_replaced_ - a temporal point is a MapPoint without a row;
a `KeyFrame` with mappoints_, a pose and countMapPoints.  The methods follow the reference's statements in order, early returns included:
  World.track_tail            Tracking::track from the decision on the mode to its return    tracking.cpp:49-116
  World.track_local_map       Tracking::trackLocalMap behind the optimisation                 tracking.cpp:276-294
  World.clear_temporal        Tracking::clearTemporalPoints                                   tracking.cpp:379-388
  World.need_new_keyframe     GMMLoc::needNewKeyFrame                                         gmmloc.cpp:324-364
  KeyFrame.count_map_points   KeyFrame::countMapPoints                                        keyframe.cpp:212-231
  World.replace_map_point     Map::replaceMapPoint, what it does to ptr_replaced_             map.cpp:112-127
  World.new_stereo_points     createMapPointsFromStereo, what it does to mappoints_           gmmloc_opt.cpp:55-63, :100
  World.update_frame_info     Map::updateFrameInfo                                            map.cpp:23-38
  World.process_frame_pose    the pose block of GMMLoc::processFrame                          gmmloc.cpp:269-292
  World.update_last_frame     Tracking::updateLastFrame                                       tracking.cpp:397-408
  World.create_temporal_points  Tracking::createTemporalPoints, what it does to mappoints_    tracking.cpp:411-465
`events` counts every branch that ran; the tests assert on it so that no comparison passes vacuously.  The float arithmetic of the
statistics is np.float32, as the reference's `float`; the poses are evaluated in the dtype of the arrays given (np.longdouble for the
derived bound of the GPU test)."""
import collections

import numpy as np

KF_NEED, KF_INTERRUPT_BA = 1, 2
BAD_REF = 1
F32 = np.float32


# ---- SE3Quat on (qx qy qz qw tx ty tz), in the dtype of its arguments
def _norm_rot(p):
    q = p[:4].copy()
    if q[3] < 0:
        q = -q
    return np.concatenate([q / np.sqrt((q * q).sum()), p[4:]])


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], dtype=a.dtype)


def _qrot(q, v):
    u = 2 * np.cross(q[:3], v)
    return v + q[3] * u + np.cross(q[:3], u)


def se3_load(p, dtype=np.float64):
    return _norm_rot(np.asarray(p, dtype))


def se3_mul(a, b):
    return _norm_rot(np.concatenate([_qmul(a[:4], b[:4]), a[4:] + _qrot(a[:4], b[4:])]))


def se3_inverse(a):
    q = np.concatenate([-a[:3], a[3:4]])
    return np.concatenate([q, _qrot(q, -a[4:])])


class MapPoint:
    __slots__ = ("row", "num_obs", "not_valid", "replaced", "pos")

    def __init__(self, row=-1, num_obs=0, not_valid=False, pos=None):
        self.row, self.num_obs, self.not_valid, self.replaced, self.pos = row, num_obs, not_valid, None, pos

    def count_observations(self):
        return self.num_obs


class KeyFrame:
    def __init__(self, row, mappoints, pose):
        self.row, self.mappoints, self.pose = row, mappoints, pose

    def count_map_points(self, minimum_obs):
        """keyframe.cpp:212-231"""
        n = 0
        check = minimum_obs > 0  # (:216)
        for mp in self.mappoints:  # (:217)
            if mp is not None:  # (:219)
                if not mp.not_valid:  # (:220)
                    if check:
                        if mp.count_observations() >= minimum_obs:  # (:222)
                            n += 1
                    else:
                        n += 1
        return n


class Frame:
    def __init__(self, mappoints, is_outlier, depth, pose=None, ref_keyframe=None):
        self.mappoints, self.is_outlier = list(mappoints), [bool(o) for o in is_outlier]
        self.depth = np.asarray(depth, F32)
        self.pose, self.T_c_r, self.ref_keyframe = pose, None, ref_keyframe

    def rows(self):
        """mappoints_ as map rows: -1 for null - and for a temporal point, which has none"""
        return np.array([-1 if mp is None else mp.row for mp in self.mappoints], np.int32)


TrackStat = collections.namedtuple("TrackStat", "res num_match_inliers ratio_map num_map num_total returned_early")


def weighted_counts(m, ba):
    """countObservations() per row from the CSR: 2 per observation with a right coordinate, 1 per monocular one, 0 for one outside the
    key-frames' tables; a range that is no sub-range of [0, NOBS]: no observation"""
    ptr, okf, ofeat, uvr = (np.asarray(a) for a in (m["obs_ptr"], m["obs_kf"], ba["obs_feat"], ba["kf_uvr"]))
    NKF, NFK = uvr.shape[:2]
    out = []
    for p in range(len(ptr) - 1):
        a, b = int(ptr[p]), int(ptr[p + 1])
        w = 0
        if 0 <= a <= b <= len(okf):
            for o in range(a, b):
                k, f = int(okf[o]), int(ofeat[o])
                if 0 <= k < NKF and 0 <= f < NFK:
                    w += 2 if uvr[k, f, 2] >= 0 else 1
        out.append(w)
    return out


class World:
    """the map's objects from its rows (m: obs_ptr, obs_kf, kf_mp, mp_valid or None, mp_pos; ba: obs_feat, kf_uvr, kf_pose)"""

    def __init__(self, m, ba, dtype=np.float64):
        self.dtype = dtype
        NMP = len(m["obs_ptr"]) - 1
        valid = np.ones(NMP, bool) if m.get("mp_valid") is None else np.asarray(m["mp_valid"]) != 0
        wc = weighted_counts(m, ba)
        pos = np.asarray(m["mp_pos"]) if m.get("mp_pos") is not None else np.zeros((NMP, 3))
        # (the header reads `countObservations() > 0` as "the CSR range is not empty"; the two differ only for a range whose observations
        #  all lie outside the key-frames' tables - the model takes well-formed maps, tests/frame_step_glue.py states the malformed ones)
        self.points = [MapPoint(p, wc[p], not valid[p], pos[p]) for p in range(NMP)]
        kf_mp = np.asarray(m["kf_mp"])
        self.keyframes = [KeyFrame(k, [self.point(int(r)) for r in kf_mp[k]], None if ba.get("kf_pose") is None else np.asarray(ba["kf_pose"])[k])
                          for k in range(kf_mp.shape[0])]
        self.events = collections.Counter()
        self.last_frame = None

    def point(self, row):
        return self.points[row] if 0 <= row < len(self.points) else None

    def keyframe(self, row):
        return self.keyframes[row] if 0 <= row < len(self.keyframes) else None

    # ---- from the chain's outputs to curr_frame_ as searchLocalPoints leaves it
    def frame_after_search(self, feat_mp, match_last, match_local, outlier, local_mp, n_local_mp, depth, last_observed=None, ref_kf=-1):
        NPcap = len(local_mp)
        nl = min(max(int(n_local_mp), 0), NPcap)
        mps = []
        for i in range(len(feat_mp)):
            j = int(match_local[i])
            r = int(local_mp[j]) if 0 <= j < nl else int(feat_mp[i])
            mp = self.point(r)
            if mp is None:
                ml = int(match_last[i])
                if last_observed is not None and 0 <= ml < len(last_observed) and not last_observed[ml]:
                    mp = MapPoint()  # a temporal point: no row, no observation
                    self.events["temporal"] += 1
            else:
                self.events["matched_local" if 0 <= j < nl else "from_last"] += 1
            mps.append(mp)
        return Frame(mps, outlier, depth, ref_keyframe=self.keyframe(int(ref_kf)))

    # ---- Tracking
    def track_local_map(self, fr):
        """tracking.cpp:276-294 behind optimizeCurrentPose"""
        n = 0
        for i in range(len(fr.mappoints)):  # (:279)
            if fr.mappoints[i] is not None:  # (:280)
                if not fr.is_outlier[i]:  # (:282)
                    if fr.mappoints[i].count_observations() > 0:  # (:285)
                        n += 1
                        self.events["inlier"] += 1
                    else:
                        self.events["inlier_unobserved"] += 1
                else:
                    self.events["outlier_temporal" if fr.mappoints[i].row < 0 else "outlier_row"] += 1
                    fr.mappoints[i] = None  # (:289)
        return n

    def clear_temporal(self, fr):
        """tracking.cpp:379-388"""
        for i in range(len(fr.mappoints)):  # (:381)
            mp = fr.mappoints[i]
            if mp is not None:  # (:383)
                if mp.count_observations() < 1:  # (:384)
                    if fr.is_outlier[i]:
                        self.events["cleared_flag_was_set"] += 1  # (never: the header's argument)
                    fr.is_outlier[i] = False  # (:385)
                    fr.mappoints[i] = None  # (:386)
                    self.events["cleared_temporal" if mp.row < 0 else "cleared_row"] += 1

    def track_tail(self, fr, mode, th_depth):
        """tracking.cpp:49-116 with the chain's mode (counts2[3]) for the two decisions the chain has taken -> TrackStat"""
        res, nmi = True, 0  # (:49)
        if mode != 0:  # (:53)
            nmi, res = 10, False  # (:54-55)
        if not res:  # (:62)
            if mode == 2:  # (:65)
                self.events["lost"] += 1
                return TrackStat(False, 10, None, 0, 0, True)  # (:66-70; last_frame_ does not advance)
        nmi = self.track_local_map(fr)  # (:81-82)
        num_map = num_total = 0  # (:88-89)
        th = F32(th_depth)
        for i in range(len(fr.mappoints)):  # (:90)
            if fr.depth[i] > F32(0) and fr.depth[i] < th:  # (:91-92)
                num_total += 1
                if fr.mappoints[i] is not None:  # (:94)
                    if fr.mappoints[i].count_observations() > 0:  # (:95)
                        num_map += 1
        ratio_map = F32(num_map) / F32(max(1, num_total))  # (:102)
        self.clear_temporal(fr)  # (:105)
        for i in range(len(fr.mappoints)):  # (:107)
            if fr.mappoints[i] is not None and fr.is_outlier[i]:  # (:108)
                fr.mappoints[i] = None
                self.events["late_outlier"] += 1  # (never: trackLocalMap took them)
        self.last_frame = fr  # (:113)
        self.events["tracked_by_keyframe" if mode == 1 else "tracked"] += 1
        return TrackStat(res, nmi, ratio_map, num_map, num_total, False)

    # ---- GMMLoc::needNewKeyFrame
    def need_new_keyframe(self, stat, ref_kf, num_kfs, frame_idx, kf_frame_idx, fps, is_idle, n_queue):
        """gmmloc.cpp:324-364 -> (num_ref_matches, verdict bits)"""
        th_ref_ratio = F32(0.4) if num_kfs < 2 else F32(0.75)  # (:327)
        th_map_ratio = F32(0.2) if stat.num_match_inliers > 300 else F32(0.35)  # (:328)
        num_obs = 2 if num_kfs <= 2 else 3  # (:331)
        kf = self.keyframe(int(ref_kf))
        num_ref = kf.count_map_points(num_obs) if kf is not None else 0  # (:332)
        c1a = F32(frame_idx) >= F32(kf_frame_idx) + F32(fps)  # (:335)
        c1b = F32(stat.num_match_inliers) < F32(num_ref) * F32(0.25) or stat.ratio_map < F32(0.3)  # (:338-339)
        c2 = (F32(stat.num_match_inliers) < F32(num_ref) * th_ref_ratio or stat.ratio_map < th_map_ratio) and stat.num_match_inliers > 15  # (:343-345)
        self.events["c1a"] += bool(c1a)
        self.events["c1b"] += bool(c1b)
        self.events["c2"] += bool(c2)
        if (c1a or c1b or is_idle) and c2:  # (:349)
            if is_idle:  # (:352)
                return num_ref, KF_NEED
            if n_queue < 3:  # (:355-358)
                return num_ref, KF_INTERRUPT_BA | KF_NEED
            return num_ref, KF_INTERRUPT_BA  # (:360)
        return num_ref, 0  # (:363)

    # ---- the mapping side, what it does to the objects this stretch reads
    def replace_map_point(self, src, tgt):
        """map.cpp:112-127"""
        if tgt.row == src.row:  # (:113)
            self.events["replace_self"] += 1
            return
        src.num_obs, src.not_valid = 0, True  # (:122-123)
        src.replaced = tgt  # (:126)
        self.events["replace"] += 1

    def note_replaced_steps(self, src_rows, tgt_rows):
        """the steps of gl_map_fuse's lists in order; a row outside the table: no such object, the step changes nothing"""
        for s, t in zip(src_rows, tgt_rows):
            ps, pt = self.point(int(s)), self.point(int(t))
            if ps is None or pt is None:
                self.events["replace_bad_row"] += 1
                continue
            self.replace_map_point(ps, pt)

    def mp_replaced(self):
        """ptr_replaced_ per row, -1 none"""
        return np.array([-1 if p.replaced is None else p.replaced.row for p in self.points], np.int32)

    def new_stereo_points(self, fr, feat_new, mp_base):
        """gmmloc_opt.cpp:55-63 and :100 as gl_create_stereo_points reports them: -2 the slot was set to null and left so, r >= 0 it
        holds the new point of row mp_base + r"""
        for i, f in enumerate(feat_new):
            if f == -2:
                fr.mappoints[i] = None
                self.events["stereo_nulled"] += 1
            elif f >= 0:
                mp = self.point(int(mp_base) + int(f))
                if mp is not None:
                    fr.mappoints[i] = mp  # (:100)
                    self.events["stereo_new"] += 1

    # ---- the hand-over
    def update_frame_info(self, fr):
        """map.cpp:23-38 -> Trc"""
        T = lambda p: se3_load(p, self.dtype)
        Trc = se3_mul(T(fr.ref_keyframe.pose), se3_inverse(T(fr.pose)))  # (:29)
        fr.T_c_r = se3_inverse(Trc)  # (:33)
        return Trc

    def process_frame_pose(self, fr, last_pose):
        """gmmloc.cpp:269-292 for data->idx >= 1 -> init_pose; fr.pose is refreshed.  last_pose: last_frame_'s Tcw, None: no such frame"""
        T = lambda p: se3_load(p, self.dtype)
        fr.pose = se3_mul(fr.T_c_r, T(fr.ref_keyframe.pose))  # (:275)
        if last_pose is None:  # (:284)
            return fr.pose  # (:285)
        delta = se3_mul(fr.pose, se3_inverse(T(last_pose)))  # (:288)
        return se3_mul(delta, fr.pose)  # (:289)

    def update_last_frame(self, fr):
        """tracking.cpp:397-408"""
        for i in range(len(fr.mappoints)):  # (:398)
            mp = fr.mappoints[i]
            if mp is not None:  # (:401)
                rep = mp.replaced  # (:402)
                if rep is not None:  # (:403)
                    fr.mappoints[i] = rep  # (:404)
                    self.events["replaced"] += 1

    def create_temporal_points(self, fr, th_depth):
        """tracking.cpp:411-465 on the last frame's objects (the caller has checked is_keyframe_, :44 / :414) -> the slots that were
        given a new temporal point.  The new point's position is not the model's business: gl_create_temporal_points has its own checker."""
        depth_indices = [(fr.depth[i], i) for i in range(len(fr.mappoints)) if fr.depth[i] > F32(0)]  # (:420-425)
        if not depth_indices:  # (:427)
            return []
        depth_indices.sort()  # (:430: by depth, then by index)
        made, num_pts = [], 0
        for z, i in depth_indices:  # (:433)
            mp = fr.mappoints[i]
            create_new = mp is None or mp.count_observations() < 1  # (:438-443)
            if create_new:
                if mp is not None:
                    self.events["temporal_over_row" if mp.row >= 0 else "temporal_over_temporal"] += 1
                    if mp.not_valid:
                        self.events["temporal_over_invalid_row"] += 1
                fr.mappoints[i] = MapPoint()  # (:451-453; feat.depth > 0 holds for every entry of the list)
                made.append(i)
            num_pts += 1  # (:457, :459)
            if z > F32(th_depth) and num_pts > 100:  # (:462)
                break
        return made

    def last_rows(self, fr):
        """the chain's last-frame rows of the frame as it stands + the held flags of createTemporalPoints (:438-443)"""
        n = len(fr.mappoints)
        out = dict(last_mp=fr.rows(), last_pt=np.zeros((n, 3)), last_valid=np.zeros(n, np.uint8), last_observed=np.zeros(n, np.uint8),
                   held=np.zeros(n, np.uint8))
        for i, mp in enumerate(fr.mappoints):
            if mp is None:
                continue
            out["last_pt"][i], out["last_valid"][i] = mp.pos, 1
            if mp.count_observations() < 1:  # (:441)
                out["held"][i] = 2
                self.events["held_unobserved"] += 1
            else:
                out["held"][i], out["last_observed"][i] = 1, 1
        return out


# ---- the three calls on arrays, through the objects
def frame_end(m, ba, feat_mp, match_last, match_local, outlier, local_mp, n_local_mp, counts2, ref_kf, last_observed, feat_depth, th_depth, rule=None,
              world=None, poison=None):
    """gl_track_frame_end for B frames -> dict(held_mp, held, stat, ratio_map, is_outlier: the model's final is_outlier_).  poison: the
    dict of outputs as they stand before the call (a lost frame keeps its rows); default: -1 / 0."""
    B, NF = np.asarray(feat_mp).shape
    W = World(m, ba) if world is None else world
    out = dict(held_mp=np.full((B, NF), -1, np.int32), held=np.zeros((B, NF), np.uint8), stat=np.zeros((B, 8), np.int32), ratio_map=np.zeros(B, F32))
    if poison is not None:
        out = {k: np.array(poison[k]) for k in out}
    is_outlier = np.array(outlier, np.uint8)
    for b in range(B):
        mode = 0 if counts2 is None else int(counts2[b][3])
        fr = W.frame_after_search(feat_mp[b], match_last[b], match_local[b], outlier[b], local_mp[b], n_local_mp[b], feat_depth[b],
                                  None if last_observed is None else last_observed[b], -1 if ref_kf is None else ref_kf[b])
        st = W.track_tail(fr, mode, th_depth)
        if st.returned_early:
            out["stat"][b] = [0, 10, 0, 0, 0, 0, 0, 0]
            continue
        nref, verdict = (0, 0) if rule is None else W.need_new_keyframe(st, ref_kf[b], **rule)
        out["held_mp"][b] = fr.rows()
        out["held"][b] = [mp is not None for mp in fr.mappoints]
        assert all(mp is None or mp.row >= 0 for mp in fr.mappoints)  # (no held point is temporal any more)
        out["stat"][b] = [int(st.res), st.num_match_inliers, st.num_map, st.num_total, nref, verdict, 0, 0]
        out["ratio_map"][b] = st.ratio_map
        is_outlier[b] = fr.is_outlier
    out["is_outlier"] = is_outlier
    return out


def note_replaced(mp_replaced, src, tgt, n=None):
    """gl_map_note_replaced -> the array afterwards: the sequential loop over rows alone (map.cpp:113, :126)"""
    rep = np.array(mp_replaced, np.int32)
    n = len(src) if n is None else min(max(int(n), 0), len(src))
    for s, t in zip(src[:n], tgt[:n]):
        s, t = int(s), int(t)
        if not (0 <= s < len(rep) and 0 <= t < len(rep)) or s == t:
            continue
        rep[s] = t
    return rep


def frame_next(m, ba, pose_tracked, pose_prev, ref_kf, held_mp, feat_new=None, mp_base=0, mp_replaced=None, dtype=np.float64, world=None,
               feat_depth=None, th_depth=None):
    """gl_track_frame_next for B frames on the map as it is -> dict(t_rc, t_cr, pose_lw, pose_cw (None rows where ref_kf is outside the
    table), held_mp, last_pt, last_valid, last_observed, held, status).  The rows of held_mp must lie in [-1, NMP).
    With feat_depth (B,NF: the FEATURES' depths - 0 in a slot that is padding on the device) and th_depth the frame is no key-frame and Tracking::createTemporalPoints follows on the same objects:
    + temp_flag (B,NF) u8 and last_mp (B,NF) i32, the frame's mappoints_ as rows AFTER it - what frame t + 1 finds in last_frame_."""
    held_mp = np.asarray(held_mp)
    B, NF = held_mp.shape
    W = World(m, ba, dtype) if world is None else world
    if mp_replaced is not None:
        for p, r in zip(W.points, mp_replaced):
            p.replaced = W.point(int(r))
    out = dict(t_rc=np.zeros((B, 7), dtype), t_cr=np.zeros((B, 7), dtype), pose_lw=np.zeros((B, 7), dtype), pose_cw=np.zeros((B, 7), dtype),
               held_mp=np.zeros((B, NF), np.int32), last_pt=np.zeros((B, NF, 3)), last_valid=np.zeros((B, NF), np.uint8),
               last_observed=np.zeros((B, NF), np.uint8), held=np.zeros((B, NF), np.uint8), status=np.zeros(B, np.int32))
    if feat_depth is not None:
        out.update(temp_flag=np.zeros((B, NF), np.uint8), last_mp=np.zeros((B, NF), np.int32))
    for b in range(B):
        fr = Frame([W.point(int(r)) for r in held_mp[b]], np.zeros(NF), np.zeros(NF), pose=pose_tracked[b], ref_keyframe=W.keyframe(int(ref_kf[b])))
        if fr.ref_keyframe is None:
            out["status"][b] = BAD_REF
        else:
            out["t_rc"][b] = W.update_frame_info(fr)
            out["t_cr"][b] = fr.T_c_r
            out["pose_cw"][b] = W.process_frame_pose(fr, None if pose_prev is None else pose_prev[b])
            out["pose_lw"][b] = fr.pose
        if feat_new is not None:
            W.new_stereo_points(fr, feat_new[b], mp_base)
        W.update_last_frame(fr)
        rows = W.last_rows(fr)
        out["held_mp"][b] = rows.pop("last_mp")
        for k, v in rows.items():
            out[k][b] = v
        if feat_depth is not None:
            fr.depth = np.asarray(feat_depth[b], F32)
            out["temp_flag"][b, W.create_temporal_points(fr, th_depth)] = 1
            out["last_mp"][b] = fr.rows()
    return out
