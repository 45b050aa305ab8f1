"""Tracking::track up to trackLocalMap (tracking.cpp:35-83) for ONE frame, restated as a small SEQUENTIAL object model on a frame dict
of synth.synth_chain_frame - the checker of tests/test_gpu_track_branches.py.  Test infrastructure; nothing in the product imports it,
and it does not import tests/chain_glue.py: that file says what the device does, this one what the reference's text does.

`Tracking` keeps what the reference keeps: a frame with mappoints_[i], is_outlier_[i] and a pose; map points with last_visible_idx_
and countObservations().  Its methods follow the reference's statements in the order they are called, early returns included:
  track                   Tracking::track                 tracking.cpp:48-72
  track_with_motion_model Tracking::trackWithMotionModel  tracking.cpp:334-377
  track_key_frame         Tracking::trackKeyFrame         tracking.cpp:297-331
  search_local_points     Tracking::searchLocalPoints     tracking.cpp:210-270
The primitives are the ORACLE's (search_by_projection_frame, search_by_bow, optimize_current_pose, project_map_points,
search_by_projection): they are held to numpy and to the device by their own tests.

The arrays name one map point up to three ways: last_pt[j], kf_pt[q] and mp_pos[l] with last_to_local[j] = l or kf_to_local[q] = l.
A `MapPoint` here is one NAME (its position and its observation count are the name's); the names of one point share the cell that
holds last_visible_idx_.

Two things are the chain's contract (gmmloc_hip.h) and not the reference's text, both marked where they happen:
  * a frame WITHOUT key-frame buffers cannot run trackKeyFrame: the chain reports ret_mm and goes on to searchLocalPoints with what
    trackWithMotionModel left (the caller owns the fallback);
  * `pose_mm`: the pose searchLocalPoints starts from may be given (the DEVICE's, equal to the model's within 1e-6) so that the search
    can be compared exactly - a projection on the very edge of a window could go either way otherwise."""
import numpy as np

TH_MM, TH_LOCAL = 7, 3  # tracking.cpp:338, :260
IDX = 7                 # curr_frame_->idx_ (>= 2: th = 3, :261)
S1_KEYS = ("feat_uv", "feat_ur", "feat_oct", "feat_angle", "feat_desc", "feat_taken", "last_pt", "last_valid", "last_oct", "last_angle", "last_desc")


class Cell:
    __slots__ = ("last_visible_idx",)

    def __init__(self):
        self.last_visible_idx = -1


class MapPoint:
    __slots__ = ("src", "k", "pos", "n_obs", "cell")

    def __init__(self, src, k, pos, n_obs, cell):
        self.src, self.k, self.pos, self.n_obs, self.cell = src, k, pos, n_obs, cell

    def count_observations(self):
        return self.n_obs


class Frame:
    __slots__ = ("idx", "mappoints", "is_outlier", "pose")


class Tracking:
    def __init__(self, o, cam, f, prm=None, scale_factor=1.2):
        self.o, self.cam, self.f, self.prm, self.sf = o, cam, f, prm, scale_factor
        NF, NL, NP = len(f["feat_oct"]), len(f["last_oct"]), len(f["mp_cand"])
        self.NF, self.NP = NF, NP
        self.has_key_frame = "kf_desc" in f
        observed = f["last_observed"] if "last_observed" in f else np.ones(NL, np.uint8)
        self.local = [MapPoint("local", l, f["mp_pos"][l], 1, Cell()) for l in range(NP)]

        def cell_of(l):
            return self.local[l].cell if 0 <= l < NP else Cell()
        self.last = [MapPoint("last", j, f["last_pt"][j], int(observed[j] != 0), cell_of(int(f["last_to_local"][j]))) for j in range(NL)]
        self.kf = []
        if self.has_key_frame:  # (a key-frame's map point is observed by that key-frame: countObservations() > 0)
            self.kf = [MapPoint("kf", q, f["kf_pt"][q], 1, cell_of(int(f["kf_to_local"][q]))) for q in range(len(f["kf_angle"]))]
        fr = self.frame = Frame()
        fr.idx, fr.mappoints, fr.is_outlier, fr.pose = IDX, [None] * NF, [False] * NF, np.array(f["pose_cw"], np.float64)
        self.drop_src, self.drop_kf = [-1] * NF, [-1] * NF
        self.n1 = self.n7 = self.nbow = self.ret_kf = self.ninl = 0
        self.retried = False

    # ---- the oracle's primitives on the model's state
    def _search_last(self, th):
        f = self.f
        m, n = self.o.search_by_projection_frame(self.cam, self.frame.pose, f["pose_lw"], *[f[k] for k in S1_KEYS], th=float(th), mono=False,
                                                 check_orientation=True, scale_factor=self.sf)
        for i in range(self.NF):
            if m[i] >= 0:
                self.frame.mappoints[i] = self.last[int(m[i])]
        return n

    def optimize_current_pose(self):
        """tracking_opt.cpp:49-217 on the frame's map points: the pose, is_outlier_ of the features with a map point (:63-69)"""
        f, fr = self.f, self.frame
        Xw, oc = np.zeros((self.NF, 3)), -np.ones(self.NF, np.int32)
        for i, mp in enumerate(fr.mappoints):
            if mp is not None:
                Xw[i], oc[i] = mp.pos, f["feat_oct"][i]
        obs = np.concatenate([f["feat_uv"], f["feat_ur"][:, None].astype(np.float64)], 1)
        pose, outl, ninl = self.o.optimize_current_pose(self.cam, fr.pose, Xw, obs, oc, prm=self.prm)
        for i, mp in enumerate(fr.mappoints):
            if mp is not None:
                fr.is_outlier[i] = bool(outl[i])
        fr.pose, self.ninl = pose, ninl
        return ninl

    # ---- the reference's statements
    def track_with_motion_model(self):
        fr = self.frame
        nmatches = self.n7 = self._search_last(TH_MM)  # (:339-340)
        if nmatches < 20:  # (:345)
            fr.mappoints = [None] * self.NF  # (:346-347)
            nmatches = self._search_last(2 * TH_MM)  # (:348)
            self.retried = True
        self.n1 = nmatches
        if nmatches < 20:  # (:352-353: before the optimisation - no pose moved, no match dropped, no point marked)
            return 0
        self.optimize_current_pose()  # (:356)
        num_matches_map = 0
        for i in range(self.NF):  # (:360-373)
            mp = fr.mappoints[i]
            if mp is not None:
                if fr.is_outlier[i]:
                    fr.mappoints[i] = None
                    fr.is_outlier[i] = False
                    mp.cell.last_visible_idx = fr.idx  # (:368)
                    self.drop_src[i] = mp.k
                    nmatches -= 1
                elif mp.count_observations() > 0:
                    num_matches_map += 1
        return num_matches_map  # (:376)

    def track_key_frame(self):
        f, fr = self.f, self.frame
        kf = dict(angle=f["kf_angle"], desc=f["kf_desc"], has_mp=f["kf_has_mp"], node_id=f["kf_node_id"], node_ptr=f["kf_node_ptr"], node_idx=f["kf_node_idx"])
        cur = dict(angle=f["feat_angle"], desc=f["feat_desc"], node_id=f["feat_node_id"], node_ptr=f["feat_node_ptr"], node_idx=f["feat_node_idx"])
        m, nmatches = self.o.search_by_bow(kf, cur, 0.7, True)  # (:300-303)
        self.nbow = nmatches
        if nmatches < 15:  # (:305-307: a log line)
            pass
        fr.mappoints = [self.kf[int(q)] if q >= 0 else None for q in m]  # (:309)
        fr.pose = np.array(f["pose_lw"], np.float64)  # (:310)
        self.optimize_current_pose()  # (:312)
        num_matches_map = 0
        for i in range(self.NF):  # (:316-329)
            mp = fr.mappoints[i]
            if mp is not None:
                if fr.is_outlier[i]:
                    fr.mappoints[i] = None
                    fr.is_outlier[i] = False
                    mp.cell.last_visible_idx = fr.idx  # (:324)
                    self.drop_kf[i] = mp.k
                    nmatches -= 1
                elif mp.count_observations() > 0:
                    num_matches_map += 1
        return num_matches_map  # (:331)

    def search_local_points(self):
        """-> (match [NF]: local map point or -1, count, in-view flags [NP]); the matches replace the frame's map points
        (orb_matcher.cpp:104)"""
        f, fr = self.f, self.frame
        for mp in fr.mappoints:  # (:213-226)
            if mp is not None:
                mp.cell.last_visible_idx = fr.idx
        cand = np.zeros(self.NP, np.uint8)
        for l, mp in enumerate(self.local):  # (:234-241; mp_cand: the caller's own exclusions, not_valid_ among them)
            if mp.cell.last_visible_idx == fr.idx:
                continue
            if f["mp_cand"][l] == 0:
                continue
            cand[l] = 1
        self.seen = np.array([mp.cell.last_visible_idx == fr.idx for mp in self.local], bool)
        taken = np.array(f["feat_taken"], np.uint8).copy()
        for i, mp in enumerate(fr.mappoints):  # (orb_matcher.cpp:74-76: a feature whose map point has observations is skipped)
            if mp is not None and mp.count_observations() > 0:
                taken[i] = 1
        twc = self.o.pose_twc(fr.pose)  # (:230)
        uvr, lvl, vc, dd, iv, n = self.o.project_map_points(self.cam, fr.pose, twc, f["mp_pos"], f["mp_normal"], f["mp_max_dist"], f["mp_min_dist"], cand,
                                                            scale_factor=self.sf)  # (:245-255)
        m, nm = np.full(self.NF, -1, np.int32), 0
        if n > 0:  # (:258-266)
            m, nm = self.o.search_by_projection(self.cam.width, self.cam.height, f["feat_uv"], f["feat_ur"], f["feat_oct"], f["feat_desc"], taken, uvr, lvl, vc,
                                                iv, f["mp_desc"], th=float(TH_LOCAL), nn_ratio=0.8, scale_factor=self.sf)
            for i in range(self.NF):
                if m[i] >= 0:
                    fr.mappoints[i] = self.local[int(m[i])]
        return m, nm, iv

    def names(self, src):
        return np.array([mp.k if (mp is not None and mp.src == src) else -1 for mp in self.frame.mappoints], np.int64)

    def track(self, pose_mm=None):
        """-> dict of what the chain reports for the frame.  mode 0: trackWithMotionModel tracked, 1: trackKeyFrame did, 2: neither
        (:66-70: the reference returns, nothing after the front means anything)."""
        res = True  # (:49)
        ret_mm = self.track_with_motion_model()  # (:51)
        mode = 0
        if ret_mm < 10:  # (:53)
            res = False
        if not res and self.has_key_frame:  # (:62; without the key-frame's buffers the chain goes on: the caller owns the fallback)
            mode = 1
            self.ret_kf = self.track_key_frame()  # (:63)
            if self.ret_kf < 10:  # (:65)
                mode = 2
        r = dict(n1=self.n1, n7=self.n7, retried=self.retried, ret_mm=ret_mm, nbow=self.nbow, ret_kf=self.ret_kf, mode=mode, ninl=self.ninl,
                 match_last=self.names("last"), match_kf=self.names("kf"), drop_src=np.array(self.drop_src, np.int64),
                 drop_kf=np.array(self.drop_kf, np.int64), pose=self.frame.pose.copy())
        if mode == 2:  # (:70)
            return r
        if pose_mm is not None:
            self.frame.pose = np.array(pose_mm, np.float64)
        m3, n3, iv = self.search_local_points()  # (:79; updateLocalMap, :77, made the frame's mp_* arrays)
        r.update(seen=self.seen, match_local=np.asarray(m3, np.int64), n3=n3, inview=iv, match_last_final=self.names("last"),
                 match_kf_final=self.names("kf"))
        return r


def track(o, cam, f, pose_mm=None, prm=None, scale_factor=1.2):
    return Tracking(o, cam, f, prm, scale_factor).track(pose_mm)


def pose_problem(f, r):
    """the edges of trackLocalMap's optimizeCurrentPose (:274) from a result of `track`: (Xw, obs, octave or -1)"""
    NF = len(f["feat_oct"])
    Xw, oc = np.zeros((NF, 3)), -np.ones(NF, np.int32)
    for i in range(NF):
        l, j, q = r["match_local"][i], r["match_last_final"][i], r["match_kf_final"][i]
        if l >= 0:
            Xw[i], oc[i] = f["mp_pos"][l], f["feat_oct"][i]
        elif j >= 0:
            Xw[i], oc[i] = f["last_pt"][j], f["feat_oct"][i]
        elif q >= 0:
            Xw[i], oc[i] = f["kf_pt"][q], f["feat_oct"][i]
    obs = np.concatenate([f["feat_uv"], f["feat_ur"][:, None].astype(np.float64)], 1)
    return Xw, obs, oc
