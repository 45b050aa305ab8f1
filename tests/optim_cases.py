"""Named scenes of a dozen points and a few key-frames on both sides of the decisions the Levenberg optimisers make (three entry points and
the anchored form of the per-frame one), built by hand in
numpy, for tests/test_optim_cases.py (CPU: the C++ oracle and oracle/numpy_ref.py both give the output each case declares) and
tests/test_gpu_optim_cases.py (every case through every launch shape of its kernel).  Test infrastructure.

The camera is CAM5 of tests/keyframe_cases.py (fx = fy = 512, cx = 256, cy = 192, bf = 64).  Poses are the identity, or RY7, the rotation by
180 degrees about y, where a key-frame must look away.  The points are the twelve of grid(): x in {-0.5, 0, 0.5}, y in {-0.25, 0.25},
z in {2, 4}, whose projections are exact - on the host and in the device's normalised coordinates alike -, so a scene without an edit has
residuals of exactly 0.0, every optimize() stops on rho == 0 after one iteration and every vertex keeps its bits.  A "plane" is a
degenerate component, a "blob" is not.  A decision on a computed quantity has a case on either side of the threshold at a relative
1e-6: one scalar of the scene (a pixel offset, a plane offset) is solved against numpy_ref (SOLVED), and the CPU test re-checks the side.
Every case declares the call, the decision, its side and every integer of the output (masks, counts; `iters` where the scene is exact:
on any other scene the last stop of optimize(40) is rounding noise), and which vertices come back unchanged BY THE BYTES.  Every case is
stable: 12 re-orderings of its edges and 36 one-ulp perturbations of its inputs leave the integers where they are and move the
oracle's pose by less than 1e-6 (checked in the CPU test; exempt: the solved scalar itself and what is listed below, and for an exact
scene `iters` and `unchanged` under the ulp probes, since one ulp on an input makes a residual non-zero).

The decisions and the reference lines (DECISIONS holds the same list; the oracle cites them in oracle/gmmloc_oracle.cpp:472-706, og_graph.hpp):

  optimizeCurrentPose (tracking_opt.cpp:21-217)                                              call "pose"
    pose.chi2_mono      :166-176  (float)chi2 > 5.991f                          5.991f (1 -/+ 1e-6), octave 0 and 2
    pose.chi2_stereo    :190-199  (float)chi2 > 7.815f                          7.815f (1 -/+ 1e-6), octave 0 and 3
    pose.float_cast     :145-146, :166  both sides of the verdict are floats    chi2 = 5.991 (1 + 1.5e-8): above the double, below the float -> inlier
    pose.mono_by_uright :67       u_right < 0 is monocular                      -0.0 and +0.0 stereo (96 px off in the third component: out); -5e-324, -1 mono
    pose.readmit        :162-164, :186-188  computeError of an outlier          A drags the pose, B is out after round 0, recomputed and in again; a B that never leaves
    pose.all_outliers_later :152-154  optimize() on what a round left           2 edges left, 3 left (the pose still converges), none left (the pose keeps its bytes)
  jointOptimization (localization_opt.cpp:456-925)                                           call "ba"; "track": gl_track_frames, P = 1
    ba.obs_chi2_mono    :799-828, :855-879  chi2 > 5.991                        (1 -/+ 1e-6) at :799, octave 0 and 2
    ba.obs_chi2_stereo  :799-828, :855-879  chi2 > 7.815                        (1 -/+ 1e-6) at :799, octave 0 and 2
    ba.float_vs_double  :806      doubles                                       the residual of pose.float_cast: erased
    ba.depth            :806, :862  !(z > 0)                                    a key-frame turned away, chi2 exactly 0: erased; turned to face: kept; fixed and free
    ba.stale_erase      :855-879  chi2 of an excluded edge is not recomputed    7.3 at :799 with the outlier that is excluded too, 4.84 recomputed: erased; a B that stays in
    ba.str_level        :773-786  chi2 > float(tri_str_thresh * ba_lambda2)     (1 -/+ 1e-6) at :773; above: excluded there and NOT dropped at :837
    ba.str_drop         :837-853  the same threshold at the end                 (1 -/+ 1e-6) at :837; above: kept at :773 and dropped; through "track": assoc -1
    ba.nondegenerate    :657-681  only a degenerate component is tested         0.3 m from a plane: excluded and dropped; from a blob: neither; through "track" too
    ba.assoc_none       :655; gl_track_frames: d2 <= 9.0                        assoc -1 against 0; d2 = 9.0 exactly (kept) and one ulp above (-1) through "track"
    ba.vertex_leaves    og_graph.hpp initializeOptimization                     a point / a free key-frame whose every observation is excluded at :799: the
                                                                                system shrinks and the vertex keeps the bits of the second round; twins that stay
    ba.pose_unobserved  og_graph.hpp initializeOptimization                     a free key-frame without an edge: its bytes; the same key-frame with three edges
    ba.single_mono      og_graph.hpp solve                                      a point with one monocular observation (a block of rank 2); with one stereo one
    ba.prior_or_fixed   :560-581  has_prior                                     on key-frame 1: a prior edge (ba_first_as_prior 1) or the vertex fixed (0)
  the fixed observers' edges of gl_track_frames_anchored (gl_ba_fast_impl.hpp: the kFixed instances of k_ba1_fast;
  gl_ba_gen.hip: k_track_pack -> k_ba_gen -> k_track_unpack)                                   call "anchored"
    fx.chi2_level       :799      stale chi2 > 5.991 / 7.815 per fixed column   (1 -/+ 1e-6), mono and stereo, octaves 0, 2, 7, F = 1 .. 4, first and last column
    fx.depth            :806, :862  !(zf > 0) in the OBSERVER's camera          an observer turned away, chi2 exactly 0: erased; facing: kept; one of three
    fx.depth_own_camera :806, :862  the frame's own depth is not the edge's     a point behind the frame and in front of both observers: their edges stay
    fx.stale_erase      :855-879  as ba.stale_erase, both on fixed observers    B in the first column (the converted case) and in the last
    fx.mono_by_uright   k_ba1_prep  u_right < 0 of a fixed observation          -0.0 and +0.0 stereo (96 px off: erased); -5e-324, -1 mono
    fx.not_observed     gl_track_anchor  fixed_oct < 0 / octave < 0             an edge, a key-frame, a key-frame turned away, a slot: the bits of the frame without it
    fx.point_keeps_fixed_edges / fx.point_leaves  initializeOptimization        the own edge excluded: one fixed edge stays; none (frozen); none but a GMM edge; F = 1 and 4
    fx.str_level / fx.str_drop  :773-786 / :837-853                             as ba.str_level / ba.str_drop with the point started ON its plane, inside the gate
    fx.prior_or_fixed   :560-581  the frame's own pose                          prior edge: moves; fixed: its bytes; neither: moves further
    fx.float_vs_double  :806      doubles                                       ba.float_vs_double with both edges on fixed observers: erased
    and, re-expressed in the dense layout by anchored_from_ba (CONVERTED), under their own keys: the eight ba_obs_chi2_*, ba_depth_fixed_*,
    ba_stale_erase*, ba_point_leaves / _stays, ba_assoc_minus_1, ba_rho_*, ba_lm_*; with twins built for this call where its own association
    (argmin + gate) would not make the case's: anc_assoc_0, anc_gate_at_9 / _above_9, anc_far_from_plane / anc_dragged_off_blob
  Levenberg (og_graph.hpp)
    lm.rho_zero         :765      rho == 0 ends optimize()                      the exact scene on all three calls: iters == 1, everything unchanged; scenes that move
    lm.reject           :748-763  a rejected trial: restored, lambda *= ni      a start 3 m off: two rejections in a row (ni reaches 8); a start accepted at once;
                                                                                on all three calls
  The stop word's three positions (:765-767, :792-796) are held by tests/test_gpu_ba.py::test_joint_optimization_stop_word: no case here.

Through gl_track_frames (call "track") the local BA's decisions have cases where the call can show them.  It returns no erase mask, but the
verdict at :799 decides what optimize(40) runs on, so the returned point tells it: ba.obs_chi2_mono / _stereo at 1 -/+ 1e-6 and ba.depth
(a point behind the frame, chi2 2e-6) declare whether point 0 ends at the centre of its blob (at_mean); the structure threshold at 1 -/+ 1e-6
declares the returned association.  The device is held to the declaration and to 1e-6 of the oracle's pose and points.

What the one-ulp probes leave alone, beyond the solved scalar: the bits a decision is ABOUT - u_right = +/-0.0 / -5e-324 in pose.mono_by_uright,
and in the gate cases the point, the mean and the covariance that make d2 = 9.0 exactly (one ulp on any of them IS the other side) -; in the
float cases both offsets +/- D_FLOAT (they are one scalar).  Pose and points of the float cases are probed like any other input.

What the entry points cannot show: in ba.vertex_leaves the vertex "comes back with the bits of the second round".  Those bits are
internal: numpy_ref's instrumentation holds them by the bytes (frozen_points / frozen_poses); the oracle and the device return only the
final value, which is held to numpy_ref's within 1e-9 (oracle) and to the oracle's within 1e-6 (device), and the device additionally to
equal bits alone and in a batch.  gl_track_frames returns no `iters`: its exact scenes declare `outer` = 3, the outer iterations of the
three optimize() together, read from the statistics buffer.

gl_track_frames_anchored returns no `iters` either (`outer` = 3 on its exact scenes, written by the on-chip route alone: the packed route
leaves the statistics buffer's second half as it was) and no verdict on the frame's OWN observation: fixed_erase is declared in full, the
own verdict is held as through gl_track_frames, by what the point does.

Decisions WITHOUT a case, and why:
  Through plain gl_track_frames (F = 0) a frame sees a point once and no erase mask comes back, so ba.float_vs_double, ba.stale_erase,
    ba.str_level apart from ba.str_drop (3.4 against 0.64 in track_str_above: one scalar crosses both) and ba.vertex_leaves /
    ba.prior_or_fixed cannot show there.  With fixed observers they can, and are built through the anchored call: fx.float_vs_double
    (measured distance of the device's chi2 from the oracle's: 0 steps of 1.52e-9 on the on-chip route, which evaluates the edge in
    normalised coordinates, and 0 steps on the packed one, against a quarter of the gap of 7.3e-9), fx.stale_erase, fx.str_level /
    fx.str_drop, fx.point_leaves / fx.point_keeps_fixed_edges, fx.prior_or_fixed.
  ba.pose_unobserved and the key-frame half of ba.vertex_leaves through either per-frame call: the one free pose sees every kept point in
    the frame's own observation, and a fixed key-frame is no vertex: no free key-frame without edges exists.  (A frame whose every own
    edge is excluded at :799 keeps the GMM edges or the prior; one with neither is the unanchored call on an empty map.)
  ba.single_mono through either per-frame call: a point seen once, monocular, exists there, but what the "ba" case declares - that
    lambda alone makes the rank-2 block solvable - shows only in where an ill-conditioned point ends (the parity tests compare such
    points at 1e-5, not 1e-6): no integer and no byte depends on it.  Held by the local BA's own cases.
  ba_far_from_blob converted: its point lies 0.3 m from a 0.1 m blob, d2 = 9 (1 - 1.3e-15): on the gate, where one ulp of an input is
    the other side.  ba.nondegenerate has anc_far_from_plane / anc_dragged_off_blob instead, the gate anc_gate_at_9 / _above_9.
  A chi2 EXACTLY at 5.991f / 7.815f after an optimisation: not reproducible, as above.  The float cases therefore use stationary scenes
    whose chi2 is exact (see FLOAT_TARGET below).
"""
import numpy as np

from oracle import numpy_ref
from tests.keyframe_cases import CAM5, ID7, REL, blob, camera, in_band, mk_map, plane  # noqa: F401 (in_band: for the tests)

f32, f64 = np.float32, np.float64
RY7 = np.array([0, 1, 0, 0, 0, 0, 0], f64)  # a rotation by 180 degrees about y: (x, y, z) -> (-x, y, -z), exactly
NCAM = numpy_ref.Cam(**CAM5)
S2I = numpy_ref.default_sigma2_inv()
TH_MONO_F, TH_STEREO_F = float(f32(5.991)), float(f32(7.815))  # the pose optimiser's thresholds: floats
TH_MONO, TH_STEREO = 5.991, 7.815                               # the local BA's: doubles
NOMAP = mk_map([blob(0.0, 0.0, -50.0)])                         # a map whose one component is 50 m behind everything: no association


class Case:
    def __init__(self, name, call, decision, side, data, want, band=None, fixed=()):
        assert decision in DECISIONS, decision
        self.name, self.call, self.decision, self.side, self.data, self.want = name, call, decision, side, data, want
        self.band = band    # dict(thr, side, q(backend)): the quantity that is compared, from what the backend returns
        self.fixed = fixed  # keys of data that the one-ulp probes leave alone (the bisected scalar lives there)

    def __repr__(self):
        return self.name


CASES = {}


def add(name, call, decision, side, data, want, **kw):
    assert name not in CASES, name
    CASES[name] = Case(name, call, decision, side, data, want, **kw)
    return name


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def grid():
    """twelve points at power-of-two depths: every projection through CAM5 and the identity is exact"""
    return np.array([[x, y, z] for z in (2.0, 4.0) for y in (-0.25, 0.25) for x in (-0.5, 0.0, 0.5)], f64)


def project(pose7, X, cam=CAM5):
    """(u, v, u_right) of the points X in the key-frame pose7 (also for a point behind it: the projection through its negative z)"""
    pc = numpy_ref.SE3.from7(pose7).map(np.asarray(X, f64))
    u = cam["fx"] * pc[..., 0] / pc[..., 2] + cam["cx"]
    v = cam["fy"] * pc[..., 1] / pc[..., 2] + cam["cy"]
    return np.stack([u, v, u - cam["bf"] / pc[..., 2]], -1)


def chi2_edge(pose7, X, uvr, octave, stereo):
    """the chi2 of one reprojection edge in the reference's expression order (types_sba / EdgeSE3ProjectXYZ*: obs - project, squared
    norm times the information)"""
    pc = numpy_ref.SE3.from7(pose7).map(np.asarray(X, f64))
    r = (np.asarray(uvr, f64) - numpy_ref.proj_stereo(pc, NCAM))[:3 if stereo else 2]
    return float(r @ (float(S2I[octave]) * np.eye(len(r))) @ r)


# ---- one face over the C++ oracle and oracle/numpy_ref ---------------------------------------------------------------------------------
def _nprm(prm):
    p = numpy_ref.Prm()
    for k, v in (prm or {}).items():
        setattr(p, k, bool(v) if k == "ba_first_as_prior" else f32(v))
    return p


def _oprm(backend, prm):
    p = type(backend.prm).from_buffer_copy(backend.prm)
    for k, v in (prm or {}).items():
        setattr(p, k, v)
    return p


def associate(backend, mean, cov, pts):
    """nearest component by Mahalanobis distance and the distance, as gl_track_frames' association step"""
    if backend is numpy_ref:
        d = numpy_ref.chi2_all(mean, numpy_ref.build_components(mean, cov)["cov_inv"], pts)
        idx = np.argmin(d, 1).astype(np.int32)
        return idx, d[np.arange(len(pts)), idx]
    h = backend.gmm_create(mean, cov.reshape(-1, 9))
    try:
        return backend.associate3d(h, pts)
    finally:
        backend.gmm_destroy(h)


def anchored_pack(data, keep, assoc, observed=lambda fo: fo >= 0):
    """the flat problem of an "anchored" frame, in the order k_track_pack documents (gl_ba_gen.hip): the kept points in slot order, per
    point the frame's own observation first, then the fixed key-frames' in index order -> (the "ba" data, [(slot, column or -1)] per observation)"""
    F = len(data["fixed_pose"])
    ptr, op, ou, oo, slot = [0], [], [], [], []
    for l in keep:
        op.append(0), ou.append(data["obs"][l]), oo.append(data["oct"][l]), slot.append((int(l), -1))
        for j in range(F):
            if observed(data["fixed_oct"][l, j]):
                op.append(1 + j), ou.append(data["fixed_obs"][l, j]), oo.append(data["fixed_oct"][l, j]), slot.append((int(l), j))
        ptr.append(len(op))
    ba = dict(mean=data["mean"], cov=data["cov"], P=1, F=F, poses=np.concatenate([data["pose"][None], np.asarray(data["fixed_pose"], f64).reshape(F, 7)]),
              prior=np.array([data["prior"]], np.uint8), points=data["Xw"][keep], assoc=assoc, obs_ptr=np.array(ptr, np.int32), obs_pose=np.array(op, np.int32),
              obs_uvr=np.array(ou, f64).reshape(-1, 3), obs_oct=np.array(oo, np.int32), prm=data.get("prm"))
    return ba, slot


def anchored_obs(data, l, j):
    """the index of the observation of slot l from fixed column j (-1: the frame's own) in the packed problem"""
    return anchored_pack(data, np.nonzero(data["oct"] >= 0)[0], None)[1].index((l, j))


def run(backend, call, data, **alt):
    """One call of a case on the oracle object or on numpy_ref -> dict of outputs, named as the device's.  alt: keyword arguments of
    numpy_ref's optimisers (one comparison altered); trace=True returns numpy_ref's instrumentation under "trace"."""
    is_np = backend is numpy_ref
    assert is_np or not alt
    want_trace = alt.pop("trace", False)
    gate = alt.pop("gate", lambda d2: d2 <= 9.0)  # (gl_track_frames' gate and the meaning of assoc < 0 live in this function:
    assoc_of = alt.pop("assoc_of", lambda a: a)    # their alterations too)
    cam = camera(CAM5)
    if call == "pose":
        if is_np:
            tr = [] if want_trace else None
            pose, outl, nin = numpy_ref.optimize_current_pose(data["pose"], data["Xw"], data["obs"], data["oct"], NCAM, _nprm(None), trace=tr, **alt)
            return dict(pose=pose, outl=outl, nin=int(nin), trace=tr)
        pose, outl, nin = backend.optimize_current_pose(cam, data["pose"], data["Xw"], data["obs"], data["oct"])
        return dict(pose=pose, outl=outl, nin=int(nin))
    mean, cov = np.ascontiguousarray(data["mean"], f64), np.ascontiguousarray(data["cov"], f64).reshape(-1, 3, 3)
    if call == "track":  # gl_track_frames: association with the gate d2 <= 9.0, then jointOptimization with one free pose
        keep = data["oct"] >= 0
        idx, d2 = associate(backend, mean, cov, data["Xw"][keep])
        a0 = np.where(gate(d2), idx, -1).astype(np.int32)
        L = int(keep.sum())
        ba = dict(mean=mean, cov=cov, P=1, F=0, poses=data["pose"][None], prior=np.zeros(1, np.uint8), points=data["Xw"][keep], assoc=a0,
                  obs_ptr=np.arange(L + 1, dtype=np.int32), obs_pose=np.zeros(L, np.int32), obs_uvr=data["obs"][keep], obs_oct=data["oct"][keep], prm=data.get("prm"))
        o = run(backend, "ba", ba, trace=want_trace, **alt) if is_np else run(backend, "ba", ba)
        assoc, dd, pts = -np.ones(len(keep), np.int32), np.zeros(len(keep)), data["Xw"].copy()
        assoc[keep], dd[keep], pts[keep] = np.where(o["dropped"] == 1, -1, a0), d2, o["points"]
        return dict(pose=o["poses"][0], points=pts, assoc=assoc, d2=dd, iters=o["iters"], trace=o.get("trace"))  # (iters: of the last optimize(40))
    if call == "anchored":  # gl_track_frames_anchored: the same association, then jointOptimization with one free pose and F fixed observers
        keep = np.nonzero(data["oct"] >= 0)[0]
        M, F = len(data["oct"]), len(data["fixed_pose"])
        idx, d2 = associate(backend, mean, cov, data["Xw"][keep])
        a0 = np.where(gate(d2), idx, -1).astype(np.int32)
        ba, slot = anchored_pack(data, keep, a0, alt.pop("observed", lambda fo: fo >= 0))
        o = run(backend, "ba", ba, trace=want_trace, **alt) if is_np else run(backend, "ba", ba)
        assoc, dd, pts = -np.ones(M, np.int32), np.zeros(M), data["Xw"].copy()
        assoc[keep], dd[keep], pts[keep] = np.where(o["dropped"] == 1, -1, a0), d2, o["points"]
        fe, own = np.zeros((M, F), np.uint8), np.zeros(M, np.uint8)
        for e, (l, j) in zip(o["erase"], slot):
            if j < 0:
                own[l] = e  # (the verdict on the frame's own observation: no output of the device's call; for the converter's check)
            else:
                fe[l, j] = e
        return dict(pose=o["poses"][0], points=pts, assoc=assoc, d2=dd, fixed_erase=fe, own_erase=own, iters=o["iters"], trace=o.get("trace"))
    assert call == "ba"
    args = (data["P"], data["F"], data["poses"], data["prior"], data["points"], assoc_of(data["assoc"]), data["obs_ptr"], data["obs_pose"], data["obs_uvr"], data["obs_oct"])
    if is_np:
        tr = {} if want_trace else None
        r = numpy_ref.joint_optimization(*args, numpy_ref.build_components(mean, cov), mean, NCAM, _nprm(data.get("prm")), trace=tr, **alt)
        return dict(poses=r[0], points=r[1], dropped=r[2], erase=r[3], iters=int(r[4]), trace=tr)
    h = backend.gmm_create(mean, cov.reshape(-1, 9))
    try:
        r = backend.joint_optimization(h, cam, *args, prm=_oprm(backend, data.get("prm")))
    finally:
        backend.gmm_destroy(h)
    return dict(poses=r[0][:data["P"]], points=r[1], dropped=r[2], erase=r[3], iters=int(r[4]))


DECISIONS = {}


def D(key, ref, what):
    DECISIONS[key] = (ref, what)


D("pose.chi2_mono", "tracking_opt.cpp:166-176", "(float)chi2 > 5.991f")
D("pose.chi2_stereo", "tracking_opt.cpp:190-199", "(float)chi2 > 7.815f")
D("pose.float_cast", "tracking_opt.cpp:145-146, :166, :190", "the cast of chi2 and of the threshold to float")
D("pose.mono_by_uright", "tracking_opt.cpp:67", "u_right < 0 makes the edge monocular")
D("pose.readmit", "tracking_opt.cpp:162-164, :186-188 (oracle :523 / :538)", "computeError of an outlier before its verdict")
D("pose.all_outliers_later", "tracking_opt.cpp:152-154", "optimize() on the level-0 edges a round left, fewer than 3 or none")
D("ba.obs_chi2_mono", "localization_opt.cpp:799-828, :855-879", "chi2 > 5.991")
D("ba.obs_chi2_stereo", "localization_opt.cpp:799-828, :855-879", "chi2 > 7.815")
D("ba.float_vs_double", "localization_opt.cpp:806", "the threshold and chi2 are doubles")
D("ba.depth", "localization_opt.cpp:806, :862 isDepthPositive", "!(z > 0) excludes and erases")
D("ba.stale_erase", "localization_opt.cpp:855-879", "e->chi2() of an excluded edge is not recomputed")
D("ba.str_level", "localization_opt.cpp:773-786", "chi2 > float(tri_str_thresh * ba_lambda2) -> level 1")
D("ba.str_drop", "localization_opt.cpp:837-853", "chi2 > float(tri_str_thresh * ba_lambda2) -> association dropped")
D("ba.nondegenerate", "localization_opt.cpp:657-681", "only a degenerate component has the structure test")
D("ba.assoc_none", "localization_opt.cpp:655; gl_track_frames d2 <= 9.0", "no GMM edge without an association")
D("ba.vertex_leaves", "og_graph.hpp initializeOptimization(level)", "a vertex without level-0 edges leaves the active set")
D("ba.pose_unobserved", "og_graph.hpp initializeOptimization(level)", "a free key-frame without edges is never active")
D("ba.single_mono", "og_graph.hpp solve", "a 3 x 3 block of rank 2 is solvable through lambda alone")
D("ba.prior_or_fixed", "localization_opt.cpp:560-581", "has_prior: an EdgeSE3QuatPrior, or the vertex fixed")
D("lm.rho_zero", "og_graph.hpp:765", "rho == 0 ends optimize()")
D("lm.reject", "og_graph.hpp:748-763", "a rejected trial is restored, lambda *= ni, ni *= 2")

# the fixed-observer edges of gl_track_frames_anchored (call "anchored"): the device's own copy of every decision on a fixed edge
D("fx.chi2_level", "localization_opt.cpp:799; gl_ba_fast_impl.hpp k_ba1_fast, phase 1 of the levels", "stale chi2 > 5.991 / 7.815 per fixed column, octaves 0, 2, 7")
D("fx.depth", "localization_opt.cpp:806, :862; k_ba1_fast !(zf > 0)", "the depth of a fixed edge in the OBSERVER's camera")
D("fx.depth_own_camera", "localization_opt.cpp:806, :862", "the frame's own depth says nothing about a fixed edge")
D("fx.stale_erase", "localization_opt.cpp:855-879; k_ba1_fast outputs", "fixed_erase reads the chi2 an excluded fixed edge was left with")
D("fx.mono_by_uright", "localization_opt.cpp:706-760; gl_ba_fast.hip k_ba1_prep", "u_right < 0 of a fixed observation is monocular")
D("fx.not_observed", "gmmloc_hip.h gl_track_anchor", "fixed_oct < 0, or octave < 0 of the slot: no edge, whatever fixed_obs holds")
D("fx.point_keeps_fixed_edges", "og_graph.hpp initializeOptimization(level)", "a point whose own edge is excluded stays active on one fixed edge")
D("fx.point_leaves", "og_graph.hpp initializeOptimization(level)", "every reprojection edge excluded: the point leaves, unless a GMM edge holds it")
D("fx.str_level", "localization_opt.cpp:773-786", "the structure threshold after the first optimize(5), with fixed observers")
D("fx.str_drop", "localization_opt.cpp:837-853", "the structure threshold at the end, with fixed observers")
D("fx.prior_or_fixed", "localization_opt.cpp:560-581", "the frame's own pose: prior edge, fixed, or free")
D("fx.float_vs_double", "localization_opt.cpp:806", "chi2 > 5.991 in doubles on a fixed edge")

P0 = np.array([0, 0, 0, 1, 0.01, 0, 0], f64)  # the start of the pose cases that are not exact: 1 cm off


def sh(uvr, du=0.0, dv=0.0, dr=0.0, mono=False):
    u = np.array(uvr, f64)
    u += (du, dv, dr)
    if mono:
        u[2] = -1.0
    return u


# ============================================================ optimizeCurrentPose ======================================================
def pose_data(pose, X=None, edits=(), octs=()):
    """the twelve exact observations, then edits: (row, du, dv, dr, mono) and octs: (row, octave)"""
    X = grid() if X is None else np.array(X, f64)
    obs = project(ID7, X)
    octv = np.zeros(len(X), np.int32)
    for (e, du, dv, dr, mono) in edits:
        obs[e] = sh(obs[e], du, dv, dr, mono)
    for (e, o) in octs:
        octv[e] = o
    return dict(pose=np.array(pose, f64), Xw=X, obs=obs, oct=octv)


def ones_but(n, *out):
    m = np.zeros(n, np.uint8)
    m[list(out)] = 1
    return m


def pose_thr_data(d, octave, mono):
    return pose_data(P0, edits=[(0, d, 0.0, 0.0, mono)], octs=[(0, octave)])


def pose_thr_q(d, octave, mono, **alt):
    """the chi2 the first round's verdict on edge 0 is taken on (all twelve edges are still in)"""
    return float(run(numpy_ref, "pose", pose_thr_data(d, octave, mono), trace=True, **alt)["trace"][0]["chi2"][0])


def secant(f, target, x0, x1, rel=2e-8):
    """x with |f(x) / target - 1| <= rel, f smooth and monotone between and around x0, x1"""
    f0, f1 = f(x0) - target, f(x1) - target
    for _ in range(40):
        if abs(f1) <= rel * abs(target):
            return x1
        x0, x1, f0 = x1, x1 - f1 * (x1 - x0) / (f1 - f0), f1
        f1 = f(x1) - target
    raise AssertionError("no convergence")


# The Levenberg runs of numpy_ref are too slow to solve 26 scalars at every import: SOLVED holds them as solved once (python -m
# tests.optim_cases prints the table again); the CPU test re-checks every one of them against its band on both implementations.
SOLVERS = {}  # name -> function that solves the scalar of the case
SOLVED = {
    "pose_chi2_mono_oct0_below": "0x1.9baf1960a5576p+1",
    "pose_chi2_mono_oct0_above": "0x1.9baf30d223bf0p+1",
    "pose_chi2_mono_oct2_below": "0x1.03d5b8afcd8e7p+2",
    "pose_chi2_mono_oct2_above": "0x1.03d5c88d1b5b9p+2",
    "pose_chi2_stereo_oct0_below": "0x1.a9765483c65edp+1",
    "pose_chi2_stereo_oct0_above": "0x1.a9766f24f1ba9p+1",
    "pose_chi2_stereo_oct3_below": "0x1.5036e2a4ec018p+2",
    "pose_chi2_stereo_oct3_above": "0x1.5036f82dcf484p+2",
    "ba_obs_chi2_mono_oct0_below": "0x1.ed867c0e737efp+1",
    "ba_obs_chi2_mono_oct0_above": "0x1.ed8690984d77ap+1",
    "ba_obs_chi2_mono_oct2_below": "0x1.1fef3a624e60dp+2",
    "ba_obs_chi2_mono_oct2_above": "0x1.1fef492b0f1b2p+2",
    "ba_obs_chi2_stereo_oct0_below": "0x1.18f6c8e43b916p+2",
    "ba_obs_chi2_stereo_oct0_above": "0x1.18f6d4a9ee488p+2",
    "ba_obs_chi2_stereo_oct2_below": "0x1.48850acb3bdc4p+2",
    "ba_obs_chi2_stereo_oct2_above": "0x1.48851bd9405bap+2",
    "ba_str_level_below": "0x1.426adb9bfcdc4p-6",
    "ba_str_drop_below": "0x1.ce599351ac5abp-4",
    "ba_str_level_above": "0x1.426a6c9dabe17p-6",
    "ba_str_drop_above": "0x1.ce59b2113e3b9p-4",
    "track_obs_chi2_mono_below": "0x1.b514561538a34p+4",
    "track_obs_chi2_mono_above": "0x1.b5145aafacedap+4",
    "track_obs_chi2_stereo_below": "0x1.368cd2912f037p+5",
    "track_obs_chi2_stereo_above": "0x1.368cd5e580dbbp+5",
    "track_str_below": "0x1.78600711e0613p-3",
    "track_str_above": "0x1.78602254af717p-3",
    "fx_chi2_mono_oct0_F1_below": "0x1.9cc02563ece52p+2",
    "fx_chi2_mono_oct0_F1_above": "0x1.9cc030008685bp+2",
    "fx_chi2_mono_oct0_F2_below": "0x1.ed867c0e60d76p+1",
    "fx_chi2_mono_oct0_F2_above": "0x1.ed8690983acc7p+1",
    "fx_chi2_mono_oct0_F3_below": "0x1.aa64d5686f47ap+1",
    "fx_chi2_mono_oct0_F3_above": "0x1.aa64e9f0e6e20p+1",
    "fx_chi2_mono_oct0_F4_below": "0x1.8c12cba49ac2ep+1",
    "fx_chi2_mono_oct0_F4_above": "0x1.8c12e191ac176p+1",
    "fx_chi2_mono_oct2_F1_below": "0x1.8eac6763fcb8bp+2",
    "fx_chi2_mono_oct2_F1_above": "0x1.8eac763c2ec15p+2",
    "fx_chi2_mono_oct2_F2_below": "0x1.1fef3a621885ep+2",
    "fx_chi2_mono_oct2_F2_above": "0x1.1fef492ad9461p+2",
    "fx_chi2_mono_oct2_F3_below": "0x1.08cad9a9fd8b1p+2",
    "fx_chi2_mono_oct2_F3_above": "0x1.08cae9a03c7e6p+2",
    "fx_chi2_mono_oct2_F4_below": "0x1.fc97e27328310p+1",
    "fx_chi2_mono_oct2_F4_above": "0x1.fc9801c42933ap+1",
    "fx_chi2_mono_oct7_F1_below": "0x1.3a33d069ab879p+3",
    "fx_chi2_mono_oct7_F1_above": "0x1.3a33e3d00c7edp+3",
    "fx_chi2_mono_oct7_F2_below": "0x1.251fd7f216d7fp+3",
    "fx_chi2_mono_oct7_F2_above": "0x1.251feab7acef8p+3",
    "fx_chi2_mono_oct7_F3_below": "0x1.2084b294f1683p+3",
    "fx_chi2_mono_oct7_F3_above": "0x1.2084c53776abbp+3",
    "fx_chi2_mono_oct7_F4_below": "0x1.1e6afcf83b6e4p+3",
    "fx_chi2_mono_oct7_F4_above": "0x1.1e6b0f5ccb90bp+3",
    "fx_chi2_stereo_oct0_F1_below": "0x1.c1ba3e57eab93p+2",
    "fx_chi2_stereo_oct0_F1_above": "0x1.c1ba4cfb5d169p+2",
    "fx_chi2_stereo_oct0_F2_below": "0x1.18f6c8de24d3fp+2",
    "fx_chi2_stereo_oct0_F2_above": "0x1.18f6d4a3d6c76p+2",
    "fx_chi2_stereo_oct0_F3_below": "0x1.e6bd6e1258f6bp+1",
    "fx_chi2_stereo_oct0_F3_above": "0x1.e6bd858a16728p+1",
    "fx_chi2_stereo_oct0_F4_below": "0x1.c44cc3d450bd1p+1",
    "fx_chi2_stereo_oct0_F4_above": "0x1.c44cdd3d5568fp+1",
    "fx_chi2_stereo_oct2_F1_below": "0x1.b737b53aa94b9p+2",
    "fx_chi2_stereo_oct2_F1_above": "0x1.b737c6d56905ap+2",
    "fx_chi2_stereo_oct2_F2_below": "0x1.48850af246d9cp+2",
    "fx_chi2_stereo_oct2_F2_above": "0x1.48851bda7bc35p+2",
    "fx_chi2_stereo_oct2_F3_below": "0x1.2e61aec188646p+2",
    "fx_chi2_stereo_oct2_F3_above": "0x1.2e61c13cf414ap+2",
    "fx_chi2_stereo_oct2_F4_below": "0x1.226db86818c98p+2",
    "fx_chi2_stereo_oct2_F4_above": "0x1.226dca4437711p+2",
    "fx_chi2_stereo_oct7_F1_below": "0x1.662ce58f20104p+3",
    "fx_chi2_stereo_oct7_F1_above": "0x1.662cfbb31d1a4p+3",
    "fx_chi2_stereo_oct7_F2_below": "0x1.4ec69de05d0b1p+3",
    "fx_chi2_stereo_oct7_F2_above": "0x1.4ec6b34e89c5bp+3",
    "fx_chi2_stereo_oct7_F3_below": "0x1.49862baff0f90p+3",
    "fx_chi2_stereo_oct7_F3_above": "0x1.498640f4a1292p+3",
    "fx_chi2_stereo_oct7_F4_below": "0x1.47203b9b3359ep+3",
    "fx_chi2_stereo_oct7_F4_above": "0x1.472050cd7de43p+3",
    "fx_str_level_below": "0x1.426d4424419fbp-6",
    "fx_str_drop_below": "0x1.ce59935189760p-4",
    "fx_str_level_above": "0x1.426cd525107ddp-6",
    "fx_str_drop_above": "0x1.ce59b21158c8bp-4",
}


def scalar(name, fn):
    SOLVERS[name] = fn
    if name not in SOLVED:
        SOLVED[name] = float(fn()).hex()
    return float.fromhex(SOLVED[name])


def pose_band_q(data, e, stereo, side):
    def q(backend):
        if side == "above":  # the edge is out after round 0; the chi2 it went out on is no output: numpy_ref's instrumentation alone
            return float(run(numpy_ref, "pose", data, trace=True)["trace"][0]["chi2"][e]) if backend is numpy_ref else None
        o = run(backend, "pose", data)
        return chi2_edge(o["pose"], data["Xw"][e], data["obs"][e], int(data["oct"][e]), stereo)
    return q


for _dec, _mono, _thr in (("pose.chi2_mono", True, TH_MONO_F), ("pose.chi2_stereo", False, TH_STEREO_F)):
    for _oct in (0, 2 if _mono else 3):
        for _side, _f in (("below", 1 - REL), ("above", 1 + REL)):
            _n = "pose_chi2_%s_oct%d_%s" % ("mono" if _mono else "stereo", _oct, _side)
            _d = scalar(_n, lambda o=_oct, m=_mono, t=_thr * _f: secant(lambda d: pose_thr_q(d, o, m), t, 3.0, 3.6))
            _data = pose_thr_data(_d, _oct, _mono)
            add(_n, "pose", _dec, _side, _data, dict(outl=ones_but(12, *([0] if _side == "above" else [])), nin=12 - (_side == "above")),
                band=dict(thr=_thr, side=_side, q=pose_band_q(_data, 0, not _mono, _side)), fixed=[("obs", (0, 0))])

# pose.mono_by_uright: the observation of point 0 is exact in u and v, its u_right is 0 - 96 px from the disparity of the point.  As a
# stereo edge that is a gross outlier, as a monocular one the residual is exactly zero
for _n, _ur, _side in (("pose_uright_minus_0", -0.0, "stereo"), ("pose_uright_plus_0", 0.0, "stereo"),
                       ("pose_uright_minus_denormal", -5e-324, "mono"), ("pose_uright_minus_1", -1.0, "mono")):
    _data = pose_data(P0)
    _data["obs"][0, 2] = _ur
    add(_n, "pose", "pose.mono_by_uright", _side, _data, dict(outl=ones_but(12, *([0] if _side == "stereo" else [])), nin=11 if _side == "stereo" else 12),
        fixed=[("obs", (0, 2))])

# pose.readmit: A (row 3, 80 px in u and u_right) drags the pose in round 0 and the monocular B (row 0, 2 px: chi2 4.0 at the clean pose)
# comes out at 7.6; in round 1 both are out, B is recomputed at the clean pose and is an inlier again.  Without the computeError B
# stays out on the 7.6 it was left with.  The twin's B (1.2 px) never goes out.
add("pose_readmit", "pose", "pose.readmit", "readmitted", pose_data(P0, edits=[(3, -80.0, 0, -80.0, False), (0, 2.0, 0, 0, True)]),
    dict(outl=ones_but(12, 3), nin=11, flag_after_round0={0: 1, 3: 1}))
add("pose_readmit_not_needed", "pose", "pose.readmit", "never out", pose_data(P0, edits=[(3, -80.0, 0, -80.0, False), (0, 1.2, 0, 0, True)]),
    dict(outl=ones_but(12, 3), nin=11, flag_after_round0={0: 0, 3: 1}))


def pairs_scene(n_exact):
    """n_exact exact stereo edges, then the next points twice each with +/- 40 px in u and u_right: at the identity the pulls of a
    pair cancel, no pose explains either, and all of them are out after round 0"""
    G = grid()
    X = [G[i] for i in range(n_exact)]
    edits = []
    for i in range(n_exact, n_exact + (12 - n_exact) // 2):
        for s in (40.0, -40.0):
            edits.append((len(X), s, 0.0, s, False))
            X.append(G[i])
    return pose_data(P0, X=X, edits=edits)


add("pose_two_edges_left", "pose", "pose.all_outliers_later", "2 left", pairs_scene(2), dict(outl=ones_but(12, *range(2, 12)), nin=2, at_identity=True))
add("pose_three_edges_left", "pose", "pose.all_outliers_later", "3 left", pairs_scene(3), dict(outl=ones_but(11, *range(3, 11)), nin=3, at_identity=True))
add("pose_no_edge_left", "pose", "pose.all_outliers_later", "0 left", pairs_scene(0), dict(outl=ones_but(12, *range(12)), nin=0, unchanged=True))

add("pose_rho_zero", "pose", "lm.rho_zero", "exact", pose_data(ID7), dict(outl=ones_but(12), nin=12, unchanged=True, q_round0=[1]))
add("pose_rho_nonzero", "pose", "lm.rho_zero", "1 cm off", pose_data(P0), dict(outl=ones_but(12), nin=12))
add("pose_lm_reject", "pose", "lm.reject", "two rejections", pose_data([0, 0, 0, 1, 0, 0, 3.0]), dict(outl=ones_but(12), nin=12, first_q=3, at_identity=True))
add("pose_lm_accept", "pose", "lm.reject", "accepted at once", pose_data(P0), dict(outl=ones_but(12), nin=12, first_q=1, at_identity=True))


# ============================================================ jointOptimization ========================================================
def ba_data(poses, P, obs, prior=None, points=None, assoc=None, gmm=None, prm=None):
    """obs: per point a list of (key-frame, (u, v, u_right), octave); key-frames [0, P) are free, the rest fixed; prior: has_prior of
    the free ones (default: key-frame 0 alone)"""
    ptr, op, ou, oo = [0], [], [], []
    for l in obs:
        for (k, u, o) in l:
            op.append(k)
            ou.append(u)
            oo.append(o)
        ptr.append(len(op))
    L = len(obs)
    mean, cov = gmm if gmm is not None else NOMAP
    d = dict(mean=mean, cov=cov, P=P, F=len(poses) - P, poses=np.array(poses, f64), prior=np.array([1] + [0] * (P - 1) if prior is None else prior, np.uint8),
             points=np.array(grid()[:L] if points is None else points, f64), assoc=np.array([-1] * L if assoc is None else assoc, np.int32),
             obs_ptr=np.array(ptr, np.int32), obs_pose=np.array(op, np.int32), obs_uvr=np.array(ou, f64).reshape(-1, 3), obs_oct=np.array(oo, np.int32))
    if prm:
        d["prm"] = prm
    return d


PR = project(ID7, grid())


def base_obs(kfs=(0, 1), L=12):
    """the first L points, each seen in stereo, exactly, by the key-frames kfs (all at the identity)"""
    return [[(k, PR[l], 0) for k in kfs] for l in range(L)]


def zeros(n, *ones):
    return ones_but(n, *ones)


def ba_thr_data(d, octave, mono):
    """key-frame 0 free with a prior, key-frames 1 and 2 fixed, all at the identity, eight points; the observation of point 0 from key-frame 1
    (row 1) is d px off in u.  Two exact observations hold the point, so the edge that is off carries four times their chi2"""
    ob = base_obs((0, 1, 2), 8)
    ob[0][1] = (1, sh(PR[0], d, mono=mono), octave)
    return ba_data([ID7, ID7, ID7], 1, ob)


def ba_thr_q(d, octave, mono):
    return float(run(numpy_ref, "ba", ba_thr_data(d, octave, mono), trace=True)["trace"]["obs_level"][1])


def ba_band_q(data, o):
    def q(backend):  # the chi2 at :799 is no output: numpy_ref's instrumentation alone; the oracle is held by its decision on either side
        return float(run(numpy_ref, "ba", data, trace=True)["trace"]["obs_level"][o]) if backend is numpy_ref else None
    return q


for _dec, _mono, _thr in (("ba.obs_chi2_mono", True, TH_MONO), ("ba.obs_chi2_stereo", False, TH_STEREO)):
    for _oct in (0, 2):
        for _side, _f in (("below", 1 - REL), ("above", 1 + REL)):
            _n = "ba_obs_chi2_%s_oct%d_%s" % ("mono" if _mono else "stereo", _oct, _side)
            _d = scalar(_n, lambda o=_oct, m=_mono, t=_thr * _f: secant(lambda d: ba_thr_q(d, o, m), t, 5.0, 7.0))
            _data = ba_thr_data(_d, _oct, _mono)
            add(_n, "ba", _dec, _side, _data, dict(dropped=zeros(8), erase=zeros(24, *([1] if _side == "above" else []))),
                band=dict(thr=_thr, side=_side, q=ba_band_q(_data, 1)), fixed=[("obs_uvr", (1, 0))])

# ba.depth: key-frame 2 is turned by 180 degrees about y and looks away from point 0; its monocular measurement is the point's projection
# through the negative z, so chi2 is exactly 0, and the observation is excluded and erased on !(z > 0) alone.  The scene is exact:
# nothing moves, every optimize() stops on rho == 0 after one iteration.  The twin's key-frame faces the point.
for _free in (False, True):
    for _pose, _side in ((RY7, "behind"), (ID7, "in front")):
        _u = sh(project(_pose, grid()[0]), mono=True)
        if not _free:
            _ob = base_obs()
            _ob[0] = _ob[0] + [(2, _u, 0)]
            _data = ba_data([ID7, ID7, _pose], 1, _ob)
        else:  # the key-frame that looks away is free (row 1) and held by a prior of its own
            _ob = base_obs((0, 2))
            _ob[0] = _ob[0] + [(1, _u, 0)]
            _data = ba_data([ID7, _pose, ID7], 2, _ob, prior=[1, 1])
        add("ba_depth_%s_%s" % ("free" if _free else "fixed", _side.replace(" ", "_")), "ba", "ba.depth", _side, _data,
            dict(dropped=zeros(12), erase=zeros(25, *([2] if _side == "behind" else [])), iters=1, unchanged=True))

# ba.stale_erase: point 0 has an exact stereo observation (key-frame 0), the monocular B 2.2 px off (key-frame 1: chi2 4.84 at the exact
# point) and the gross outlier A (key-frame 2, -30 px).  Under the robust kernel A drags the point, B is at 7.3 at :799 and is excluded
# with A; the point returns, B would be at 4.84 - and is erased on the 7.3 it was left with.  The twin's B is 1 px off and stays in.
for _n, _dB, _side, _er in (("ba_stale_erase", 2.2, "erased on the stale chi2", (1, 2)), ("ba_stale_erase_not_excluded", 1.0, "kept", (2,))):
    _ob = base_obs()
    _ob[0] = [(0, PR[0], 0), (1, sh(PR[0], _dB, mono=True), 0), (2, sh(PR[0], -30.0, 0, -30.0), 0)]
    add(_n, "ba", "ba.stale_erase", _side, ba_data([ID7, ID7, ID7], 1, _ob), dict(dropped=zeros(12), erase=zeros(25, *_er)))


# ba.str_level / ba.str_drop: point 1 = (0, -0.25, 2) is associated with a plane at z = 2 + p; ba_lambda2 = 100, so the threshold is
# float(0.0064f * 100f) = 0.64, a distance of 0.08 m.  The outlying observations want the point at z = 4 (u_right 16 px off).
STR_PRM = dict(ba_lambda2=100.0)
TH_STR100 = float(f32(f32(0.0064) * f32(100.0)))


def str_a_data(p):
    """(a) three exact stereo observations (key-frames 0, 1, 2) and two outlying ones (3, 4): after the first optimize(5) the outliers
    hold the point 0.1 m behind z = 2; the plane sits near where they hold it.  At :799 both outliers go, and the point returns to z = 2"""
    ob = base_obs()
    ob[1] = [(0, PR[1], 0), (1, PR[1], 0), (2, PR[1], 0), (3, sh(PR[1], dr=16.0), 0), (4, sh(PR[1], dr=16.0), 0)]
    a = [-1] * 12
    a[1] = 0
    return ba_data([ID7] * 5, 1, ob, assoc=a, gmm=mk_map([plane(0.0, -0.25, 2.0 + p), blob(0.0, 0.0, -50.0)]), prm=STR_PRM)


def str_b_data(p):
    """(b) two exact stereo observations (key-frames 0, 1) and one outlying one (2) that pulls the point towards the plane at z = 2 + p:
    at :773 the point is near the plane, after the outlier is gone at :799 it settles between the plane and z = 2"""
    ob = base_obs()
    ob[1] = [(0, PR[1], 0), (1, PR[1], 0), (2, sh(PR[1], dr=16.0), 0)]
    a = [-1] * 12
    a[1] = 0
    return ba_data([ID7] * 3, 1, ob, assoc=a, gmm=mk_map([plane(0.0, -0.25, 2.0 + p), blob(0.0, 0.0, -50.0)]), prm=STR_PRM)


def str_q(data, key):
    return float(run(numpy_ref, "ba", data, trace=True)["trace"][key][1])


def str_band_q(data, key):
    def q(backend):
        if key == "str_level":  # the chi2 after the first optimize(5) is no output
            return str_q(data, key) if backend is numpy_ref else None
        z = run(backend, "ba", data)["points"][1][2]
        return 100.0 * (z - data["mean"][0][2]) ** 2
    return q


for _side, _f in (("below", 1 - REL), ("above", 1 + REL)):
    _p = scalar("ba_str_level_" + _side, lambda t=TH_STR100 * _f: secant(lambda p: str_q(str_a_data(p), "str_level"), t, 0.02, 0.03))
    _data = str_a_data(_p)
    # excluded at :773 (above) and NOT dropped at :837: with the edge out the point ends at z = 2, |p| < 0.08 from the plane; kept (below):
    # the point ends between z = 2 and the plane
    add("ba_str_level_" + _side, "ba", "ba.str_level", _side, _data, dict(dropped=zeros(12), erase=zeros(27, 5, 6), at_exact={1: _side == "above"}),
        band=dict(thr=TH_STR100, side=_side, q=str_band_q(_data, "str_level")), fixed=[("mean", (0, 2))])
    _p = scalar("ba_str_drop_" + _side, lambda t=TH_STR100 * _f: secant(lambda p: str_q(str_b_data(p), "str_drop"), t, 0.09, 0.10))
    _data = str_b_data(_p)
    # kept at :773 (the outlier holds the point near the plane) and dropped at :837 (above)
    add("ba_str_drop_" + _side, "ba", "ba.str_drop", _side, _data, dict(dropped=zeros(12, *([1] if _side == "above" else [])), erase=zeros(25, 4), at_exact={1: False}),
        band=dict(thr=TH_STR100, side=_side, q=str_band_q(_data, "str_drop")), fixed=[("mean", (0, 2))])

# ba.nondegenerate: point 1 0.3 m from its component.  A plane: excluded and dropped.  A blob: the same offset, never either
for _n, _comp, _side, _dr in (("ba_far_from_plane", plane, "degenerate", (1,)), ("ba_far_from_blob", blob, "not degenerate", ())):
    _a = [-1] * 12
    _a[1] = 0
    add(_n, "ba", "ba.nondegenerate", _side, ba_data([ID7, ID7], 1, base_obs(), assoc=_a, gmm=mk_map([_comp(0.0, -0.25, 2.3), blob(0.0, 0.0, -50.0)])),
        dict(dropped=zeros(12, *_dr), erase=zeros(24)))

# ba.assoc_none: the exact scene with a plane 1 cm behind point 1.  Associated, the point moves; with assoc = -1 there is no edge and the scene stays exact
for _n, _a1, _side in (("ba_assoc_minus_1", -1, "none"), ("ba_assoc_0", 0, "associated")):
    _a = [-1] * 12
    _a[1] = _a1
    _w = dict(dropped=zeros(12), erase=zeros(24))
    if _a1 < 0:
        _w.update(iters=1, unchanged=True)
    else:
        _w.update(moved_points=[1])
    add(_n, "ba", "ba.assoc_none", _side, ba_data([ID7, ID7], 1, base_obs(), assoc=_a, gmm=mk_map([plane(0.0, -0.25, 2.01), blob(0.0, 0.0, -50.0)])), _w)

# ba.vertex_leaves (point): point 0 has two observations no position explains (+40 px monocular, -40 px and +40 px of disparity): both are
# excluded at :799 and the point has no level-0 edge in optimize(40): it keeps the bits the second optimize(5) left
_ob = base_obs()
_ob[0] = [(0, sh(PR[0], 40.0, mono=True), 0), (1, sh(PR[0], -40.0, 0, 40.0), 0)]
add("ba_point_leaves", "ba", "ba.vertex_leaves", "point without edges", ba_data([ID7, ID7], 1, _ob), dict(dropped=zeros(12), erase=zeros(24, 0, 1), n_last=39, n_shrinks=True, frozen_points=[0]))
_ob = base_obs()
_ob[0] = [(0, sh(PR[0], 40.0, mono=True), 0), (1, sh(PR[0], 1.0), 0)]
add("ba_point_stays", "ba", "ba.vertex_leaves", "point keeps an edge", ba_data([ID7, ID7], 1, _ob), dict(dropped=zeros(12), erase=zeros(24, 0), n_last=42))
# ba.vertex_leaves (key-frame): the free key-frame 1 (no prior) sees six points, each 40 px off in another direction and against its
# disparity: every one (octave 4, so that it pulls less at the points) is excluded at :799 and the key-frame keeps the pose the second optimize(5) left
_ob = [[(0, PR[l], 0), (2, PR[l], 0)] for l in range(12)]
_kf1 = []
for _l, (_du, _dv, _dr) in zip((0, 2, 4, 7, 9, 11), ((40, 40, -40), (-40, 40, 40), (40, -40, -40), (-40, -40, 40), (40, 0, -40), (0, -40, 40))):
    _ob[_l] = _ob[_l] + [(1, sh(PR[_l], _du, _dv, _dr), 4)]
    _kf1.append(sum(len(x) for x in _ob[:_l + 1]) - 1)
add("ba_keyframe_leaves", "ba", "ba.vertex_leaves", "key-frame without edges", ba_data([ID7, ID7, ID7], 2, _ob), dict(dropped=zeros(12), erase=zeros(30, *_kf1), n_last=42, n_shrinks=True, frozen_poses=[1]))
add("ba_keyframe_stays", "ba", "ba.vertex_leaves", "key-frame keeps its edges", ba_data([ID7, ID7, ID7], 2, [[(0, PR[l], 0), (2, PR[l], 0)] + ([(1, sh(PR[l], 1.0, 0, 1.0), 0)] if l in (0, 2, 4, 7, 9, 11) else []) for l in range(12)]),
    dict(dropped=zeros(12), erase=zeros(30), n_last=48, moved_poses=[1]))

# ba.pose_unobserved: the free key-frame 1 has no observation and no prior from the start; one observation is 3 px off so that the rest moves
_ob = [[(0, PR[l], 0), (2, PR[l], 0)] for l in range(12)]
_ob[0][1] = (2, sh(PR[0], 3.0), 0)
add("ba_pose_unobserved", "ba", "ba.pose_unobserved", "no edge", ba_data([ID7, RY7, ID7], 2, _ob), dict(dropped=zeros(12), erase=zeros(24), unchanged_poses=[1], moved_points=[0]))
_ob = [[(0, PR[l], 0), (2, PR[l], 0)] for l in range(12)]
_ob[0][1] = (2, sh(PR[0], 3.0), 0)
_ob[5] = _ob[5] + [(1, sh(PR[5], 1.0, 0, 1.0), 0)]
_ob[6] = _ob[6] + [(1, sh(PR[6], 1.0, 0, 1.0), 0)]
_ob[10] = _ob[10] + [(1, sh(PR[10], 1.0, 0, 1.0), 0)]
add("ba_pose_observed", "ba", "ba.pose_unobserved", "three edges", ba_data([ID7, ID7, ID7], 2, _ob), dict(dropped=zeros(12), erase=zeros(27), moved_poses=[1]))

# ba.single_mono: point 5 is seen once, monocular, 1 px off: J^T J has rank 2 and only lambda makes its block solvable
_ob = base_obs()
_ob[5] = [(1, sh(PR[5], 1.0, mono=True), 0)]
_ob[0][1] = (1, sh(PR[0], 3.0), 0)
add("ba_single_mono", "ba", "ba.single_mono", "one mono edge", ba_data([ID7, ID7], 1, _ob), dict(dropped=zeros(12), erase=zeros(23), moved_points=[0, 5]))
_ob = base_obs()
_ob[5] = [(1, sh(PR[5], 1.0), 0)]
_ob[0][1] = (1, sh(PR[0], 3.0), 0)
add("ba_single_stereo", "ba", "ba.single_mono", "one stereo edge", ba_data([ID7, ID7], 1, _ob), dict(dropped=zeros(12), erase=zeros(23), moved_points=[0, 5]))

# ba.prior_or_fixed: has_prior on key-frame 1 (not row 0), whose eight observations are 1 px off in u and u_right
for _fp in (1, 0):
    _ob = [[(0, PR[l], 0), (1, sh(PR[l], 1.0, 0, 1.0), 0), (2, PR[l], 0)] for l in range(8)]
    _w = dict(dropped=zeros(8), erase=zeros(24))
    _w.update(dict(moved_poses=[1]) if _fp else dict(unchanged_poses=[1]))
    add("ba_prior_row1_as_%s" % ("prior" if _fp else "fixed"), "ba", "ba.prior_or_fixed", "prior edge" if _fp else "fixed", ba_data([ID7, ID7, ID7], 2, _ob, prior=[0, 1], prm=dict(ba_first_as_prior=_fp)), _w)

add("ba_rho_zero", "ba", "lm.rho_zero", "exact", ba_data([ID7, ID7], 1, base_obs()), dict(dropped=zeros(12), erase=zeros(24), iters=1, unchanged=True))
_ob = base_obs()
_ob[0][1] = (1, sh(PR[0], 3.0), 0)
add("ba_rho_nonzero", "ba", "lm.rho_zero", "3 px off", ba_data([ID7, ID7], 1, _ob), dict(dropped=zeros(12), erase=zeros(24), moved_points=[0]))

# lm.reject on the local BA: the free key-frame 0 (no prior) starts 3 m off along z; key-frame 1 is fixed.  The first trial is rejected twice
for _n, _tz, _side, _q in (("ba_lm_reject", 3.0, "two rejections", 3), ("ba_lm_accept", 1.0, "accepted at once", 1)):
    add(_n, "ba", "lm.reject", _side, ba_data([np.array([0, 0, 0, 1, 0, 0, _tz], f64), ID7], 1, base_obs(), prior=[0]),
        dict(dropped=zeros(12), erase=zeros(24), first_q=_q, at_identity=True))

# pose.float_cast / ba.float_vs_double: the same residual on either optimiser.  chi2 = 5.991 (1 + 1.5e-8) lies above the double 5.991 and
# below the float 5.991f = 5.991 (1 + 2.93e-8): (float)chi2 > 5.991f is false in the pose optimiser, chi2 > 5.991 is true in the local BA.
# A chi2 that an optimisation ends on is not reproducible to 1e-8 (the Levenberg schedule stops where its budget ends: along a ladder of
# 1e-9 steps of one offset the ORACLE's own verdict flipped back and forth), so these scenes do not optimise: point 0 is seen twice,
# D_FLOAT px off in u to either side, monocular, octave 0.  The two pulls cancel bit for bit (D_FLOAT has 40 fractional bits, so
# 128 +/- D_FLOAT and the residuals are exact), the start is a stationary point, optimize() stops on rho == 0, and both edges have
# chi2 = D_FLOAT^2 exactly, in any expression order.
# Measured on the MI355X (test_gpu_optim_cases.py::test_float_gap_distance): moving D_FLOAT in steps of 2^-29 px (1.52e-9 of chi2), the device's
# verdict flips on the same step as the oracle's in both optimisers and, on a fixed observer's edge of gl_track_frames_anchored, on the on-chip
# route (normalised coordinates) and on the packed one (step -9 each, distance 0 steps): its chi2 is within 1.52e-9 of the oracle's, against a quarter of the gap of 7.3e-9.
# (fx = 512 is a power of two and the octave is 0: the device's normalised-coordinate chi2 is this chi2 bit for bit, so the figure is about
# the comparison - cast, constant, strictness -, not about the expression order on another camera.)
FLOAT_TARGET = TH_MONO * (1 + 1.5e-8)
GAP = TH_MONO_F / TH_MONO - 1
D_FLOAT = float(np.round(np.sqrt(FLOAT_TARGET) * 2.0 ** 40) / 2.0 ** 40)
FLOAT_STEP = 2.0 ** -29  # of the offset; 2 * FLOAT_STEP / D_FLOAT = 1.52e-9 of chi2


def pose_float_data(d):
    G = grid()
    return pose_data(ID7, X=list(G) + [G[0]], edits=[(0, d, 0.0, 0.0, True), (12, -d, 0.0, 0.0, True)])


def ba_float_data(d):
    ob = base_obs((0, 1, 2), 8)
    ob[0] = [(0, PR[0], 0), (1, sh(PR[0], d, mono=True), 0), (2, sh(PR[0], -d, mono=True), 0)]
    return ba_data([ID7, ID7, ID7], 1, ob)


def in_float_gap(q):
    """the target of the two float cases: within a quarter of the gap between 5.991 and 5.991f of 5.991 (1 + 1.5e-8)"""
    return abs(q / FLOAT_TARGET - 1) <= GAP / 4


assert in_float_gap(D_FLOAT * D_FLOAT) and abs(D_FLOAT * D_FLOAT / FLOAT_TARGET - 1) < 1e-12
add("pose_float_cast", "pose", "pose.float_cast", "between the double and the float", pose_float_data(D_FLOAT), dict(outl=ones_but(13), nin=13, unchanged=True, q_round0=[1]),
    band=dict(thr=TH_MONO, side="float", q=lambda b: float(run(numpy_ref, "pose", pose_float_data(D_FLOAT), trace=True)["trace"][0]["chi2"][0]) if b is numpy_ref else None),
    fixed=[("obs", (0, 0)), ("obs", (12, 0))])
add("pose_float_cast_above_both", "pose", "pose.float_cast", "above both", pose_float_data(D_FLOAT + 64 * FLOAT_STEP), dict(outl=ones_but(13, 0, 12), nin=11, unchanged=True),
    fixed=[("obs", (0, 0)), ("obs", (12, 0))])
add("ba_float_vs_double", "ba", "ba.float_vs_double", "between the double and the float", ba_float_data(D_FLOAT), dict(dropped=zeros(8), erase=zeros(24, 1, 2), iters=1, unchanged=True),
    band=dict(thr=TH_MONO, side="float", q=lambda b: float(run(numpy_ref, "ba", ba_float_data(D_FLOAT), trace=True)["trace"]["obs_level"][1]) if b is numpy_ref else None),
    fixed=[("obs_uvr", (1, 0)), ("obs_uvr", (2, 0))])
add("ba_float_vs_double_below_both", "ba", "ba.float_vs_double", "below both", ba_float_data(D_FLOAT - 64 * FLOAT_STEP), dict(dropped=zeros(8), erase=zeros(24), iters=1, unchanged=True),
    fixed=[("obs_uvr", (1, 0)), ("obs_uvr", (2, 0))])


def float_probe(name, ks):
    """the data of a float case with its offset moved by k * FLOAT_STEP for the k in ks: the step at which the verdict of an
    implementation flips tells where it puts chi2 against its threshold"""
    mk = pose_float_data if name.startswith("pose") else ba_float_data  # ("anc_float_vs_double": the "ba" data, for anchored_from_ba)
    return [mk(D_FLOAT + k * FLOAT_STEP) for k in ks]


# ============================================================ gl_track_frames ==========================================================
def anchors(skip=()):
    """a blob of 0.1 m exactly at every grid point but those in skip: zero residual, and what removes the gauge freedom of one free pose"""
    G = grid()
    return [blob(*G[l]) for l in range(12) if l not in skip]


def track_data(comps, X=None, edits=()):
    d = pose_data(ID7, X=X, edits=edits)
    d["obs"] = project(ID7, d["Xw"])
    for (e, du, dv, dr, mono) in edits:
        d["obs"][e] = sh(d["obs"][e], du, dv, dr, mono)
    d["mean"], d["cov"] = mk_map(comps)
    return d


add("track_rho_zero", "track", "lm.rho_zero", "exact", track_data(anchors()), dict(assoc=np.arange(12, dtype=np.int32), outer=3, unchanged=True))
add("track_rho_zero_no_association", "track", "lm.rho_zero", "exact", track_data([blob(0.0, 0.0, -50.0)]), dict(assoc=-np.ones(12, np.int32), outer=3, unchanged=True))
add("track_rho_nonzero", "track", "lm.rho_zero", "3 px off", track_data(anchors(), edits=[(0, 3.0, 0, 0, False)]), dict(assoc=np.arange(12, dtype=np.int32), moved_points=[0]))

for _n, _tz, _side, _q in (("track_lm_reject", 3.0, "two rejections", 3), ("track_lm_accept", 1.0, "accepted at once", 1)):
    _d = track_data(anchors())
    _d["pose"] = np.array([0, 0, 0, 1, 0, 0, _tz], f64)
    add(_n, "track", "lm.reject", _side, _d, dict(assoc=np.arange(12, dtype=np.int32), first_q=_q, at_identity=True))

# ba.assoc_none through the gate d2 <= 9.0: point 5 is moved to (3, 0.25, 8), exactly 3 sigma from a unit-covariance component at
# (0, 0.25, 8) (component 11; the eleven anchors are 0 - 10): d2 = 9.0 exactly and the association is kept; one ulp farther it is not
for _n, _x, _side in (("track_gate_at_9", 3.0, "d2 = 9.0"), ("track_gate_above_9", float(np.nextafter(3.0, 4.0)), "d2 > 9.0")):
    _X = grid()
    _X[5] = (_x, 0.25, 8.0)
    _a = np.array([0, 1, 2, 3, 4, 11 if _x == 3.0 else -1, 5, 6, 7, 8, 9, 10], np.int32)
    add(_n, "track", "ba.assoc_none", _side, track_data(anchors(skip=(5,)) + [blob(0.0, 0.25, 8.0, 1.0)], X=_X), dict(assoc=_a, d2_of={5: 9.0} if _x == 3.0 else {}),
        fixed=[("Xw", (5, 0)), ("Xw", (5, 1)), ("Xw", (5, 2)), ("mean", None), ("cov", None)])

# ba.str_drop / ba.nondegenerate through gl_track_frames: a dropped association comes back as -1.  Point 1 starts ON its component (the
# gate passes with d2 = 0), its observation is that of a point 0.3 m deeper (ba_lambda2 = 100): against a plane it ends 0.2 m off and the association
# is dropped, against a blob at the same place nothing is
for _n, _comp, _dec, _side in (("track_dragged_off_plane", plane, "ba.str_drop", "dropped"), ("track_dragged_off_blob", blob, "ba.nondegenerate", "kept")):
    _c = anchors()
    _c[1] = _comp(0.0, -0.25, 2.0)
    _a = np.arange(12, dtype=np.int32)
    if _comp is plane:
        _a[1] = -1
    _d = track_data(_c)
    _d["obs"][1] = project(ID7, np.array([0.0, -0.25, 2.3]))
    _d["prm"] = STR_PRM
    add(_n, "track", _dec, _side + " (track)", _d, dict(assoc=_a))


# ba.obs_chi2_* / ba.depth / the structure threshold through gl_track_frames.  The call returns no erase mask, but the verdict at :799 decides
# what optimize(40) runs on: every point sits on a tight blob (0.011 m: not degenerate, 8 264 / m^2 against the 65 536 / m^2 of a
# reprojection edge at z = 2), so the pose is held, and the observation of point 0 is d px off.  Kept at :799, the point ends 0.06 m
# off its blob; excluded, it returns to the blob's centre to rounding, and the pose to the identity (declared: at_mean).
def tight():
    G = grid()
    return [blob(*G[l], 0.011) for l in range(12)]


def track_obs_data(d, mono):
    return track_data(tight(), edits=[(0, d, 0.0, 0.0 if mono else d, mono)])


def track_q(data, key, i):
    return float(run(numpy_ref, "track", data, trace=True)["trace"][key][i])


for _mono, _dec, _thr, _x0, _x1 in ((True, "ba.obs_chi2_mono", TH_MONO, 23.0, 24.0), (False, "ba.obs_chi2_stereo", TH_STEREO, 33.0, 34.0)):
    for _side, _f in (("below", 1 - REL), ("above", 1 + REL)):
        _n = "track_obs_chi2_%s_%s" % ("mono" if _mono else "stereo", _side)
        _d = scalar(_n, lambda m=_mono, t=_thr * _f, a=_x0, b=_x1: secant(lambda d: track_q(track_obs_data(d, m), "obs_level", 0), t, a, b))
        _data = track_obs_data(_d, _mono)
        add(_n, "track", _dec, _side + " (track)", _data, dict(assoc=np.arange(12, dtype=np.int32), at_mean={0: _side == "above"}),
            band=dict(thr=_thr, side=_side, q=lambda b, _data=_data: track_q(_data, "obs_level", 0) if b is numpy_ref else None),
            fixed=[("obs", (0, 0))] + ([] if _mono else [("obs", (0, 2))]))

# ba.depth through gl_track_frames: point 0 is BEHIND the frame, its monocular measurement the projection through the negative z; its blob is
# centred 1 cm beside it, so chi2 at :799 is 2e-6, not 0, and the edge goes on !(z > 0) alone: the point ends at the blob's centre.
# The twin is in front: the edge stays and holds the point 0.5 mm from where it started
for _n, _z, _side in (("track_depth_behind", -2.0, "behind (track)"), ("track_depth_in_front", 2.0, "in front (track)")):
    _X = grid()
    _X[0] = (-0.5, -0.25, _z)
    _c = tight()
    _c[0] = blob(-0.49, -0.25, _z, 0.011)
    _d = track_data(_c, X=_X)
    _d["obs"][0, 2] = -1.0
    add(_n, "track", "ba.depth", _side, _d, dict(assoc=np.arange(12, dtype=np.int32), at_mean={0: _z < 0}))


# the structure threshold through gl_track_frames (ba_lambda2 = 100: 0.64): point 1 starts on its plane, its observation is that of a point dz
# deeper.  With one observation per point nothing can be removed between :773 and :837, so ONE scalar crosses both: below, the
# edge is kept at both and the association stays; above, it is excluded at :773 (the band is taken there), the point follows its
# observation, and the association is dropped at :837
def track_str_data(dz):
    c = anchors()
    c[1] = plane(0.0, -0.25, 2.0)
    d = track_data(c)
    d["obs"][1] = project(ID7, np.array([0.0, -0.25, 2.0 + dz]))
    d["prm"] = STR_PRM
    return d


for _side, _f in (("below", 1 - REL), ("above", 1 + REL)):
    _n = "track_str_" + _side
    _dz = scalar(_n, lambda t=TH_STR100 * _f: secant(lambda dz: track_q(track_str_data(dz), "str_level", 1), t, 0.17, 0.18))
    _data = track_str_data(_dz)
    _a = np.arange(12, dtype=np.int32)
    if _side == "above":
        _a[1] = -1
    add(_n, "track", "ba.str_drop", _side + " (track)", _data, dict(assoc=_a),
        band=dict(thr=TH_STR100, side=_side, q=lambda b, _data=_data: track_q(_data, "str_level", 1) if b is numpy_ref else None), fixed=[("obs", (1, 2))])


# ============================================================ gl_track_frames_anchored =================================================
# The dense layout of the entry point: pose (7), Xw / obs (M x 3), oct (M), prior (0 / 1), fixed_pose (F x 7), fixed_obs (M x F x 3),
# fixed_oct (M x F; < 0: not observed), mean, cov, prm.  The high-precision statement is jointOptimization(P = 1, F fixed) on the
# problem anchored_pack() builds.  Outputs: pose, points, assoc (-1 where dropped or ungated), d2, fixed_erase (M x F).
def anchored_from_ba(data):
    """a "ba" case in the dense layout -> (data, [(slot, column or -1)] per observation of the "ba" case).  Needs P == 1, every point seen
    exactly once by key-frame 0 and at most once by a fixed one, and the call's own association (argmin + gate on the case's map) to
    reproduce the case's."""
    assert data["P"] == 1
    L, F = len(data["points"]), data["F"]
    d = dict(pose=data["poses"][0].copy(), Xw=data["points"].copy(), obs=np.zeros((L, 3)), oct=-np.ones(L, np.int32), prior=int(data["prior"][0]),
             fixed_pose=data["poses"][1:].copy(), fixed_obs=np.zeros((L, F, 3)), fixed_oct=-np.ones((L, F), np.int32), mean=data["mean"], cov=data["cov"])
    if data.get("prm"):
        d["prm"] = data["prm"]
    slot = []
    for l in range(L):
        for o in range(data["obs_ptr"][l], data["obs_ptr"][l + 1]):
            k = int(data["obs_pose"][o])
            if k == 0:
                assert d["oct"][l] < 0
                d["obs"][l], d["oct"][l] = data["obs_uvr"][o], data["obs_oct"][o]
            else:
                assert d["fixed_oct"][l, k - 1] < 0
                d["fixed_obs"][l, k - 1], d["fixed_oct"][l, k - 1] = data["obs_uvr"][o], data["obs_oct"][o]
            slot.append((l, k - 1))
        assert d["oct"][l] >= 0, "a point the frame itself does not see"
    idx, d2 = associate(numpy_ref, np.asarray(d["mean"], f64), np.asarray(d["cov"], f64).reshape(-1, 3, 3), d["Xw"])
    assert np.array_equal(np.where(d2 <= 9.0, idx, -1), data["assoc"]), "the call's own association is not the case's"
    return d, slot


def fe_of(L, F, *ones):
    m = np.zeros((L, F), np.uint8)
    for l, j in ones:
        m[l, j] = 1
    return m


def anc_q(data, key, l, j=None):
    """numpy_ref's instrumentation of an "anchored" case: the chi2 a verdict was taken on, for the observation of slot l from column j
    (obs_level) or for point l (str_level, str_drop)"""
    def q(backend):
        if backend is not numpy_ref:
            return None
        return float(run(numpy_ref, "anchored", data, trace=True)["trace"][key][l if j is None else anchored_obs(data, l, j)])
    return q


CONVERTED = {}  # name of the "anchored" case -> (name of the "ba" case, its observations' (slot, column))
KEEP_WANT = ("iters", "unchanged", "moved_points", "at_identity", "first_q", "n_last", "n_shrinks", "frozen_points")


def convert(ba_name, decision=None):
    c = CASES[ba_name]
    d, slot = anchored_from_ba(c.data)
    L, F = d["fixed_oct"].shape
    w = {k: v for k, v in c.want.items() if k in KEEP_WANT}
    w["assoc"] = np.where(c.want["dropped"][:L] == 1, -1, c.data["assoc"]).astype(np.int32)
    w["fixed_erase"] = fe_of(L, F, *[s for o, s in enumerate(slot) if s[1] >= 0 and c.want["erase"][o]])
    if "at_exact" in c.want:
        w["at_exact"] = {l: (c.data["points"][l], v) for l, v in c.want["at_exact"].items()}
    if w.get("iters") == 1:
        w["outer"] = 3
    if d["prior"] and not (d.get("prm") or {}).get("ba_first_as_prior", 1):
        w["pose_bytes"] = True
    fixed = []
    for k, i in c.fixed:
        if k == "obs_uvr":
            l, j = slot[i[0]]
            fixed.append(("obs", (l, i[1])) if j < 0 else ("fixed_obs", (l, j, i[1])))
        else:
            fixed.append((k, i))
    band = None
    if c.band:  # (every banded case that is converted takes its band at :799, on one observation)
        o = [i for k, i in c.fixed if k == "obs_uvr"][0][0]
        band = dict(thr=c.band["thr"], side=c.band["side"], q=anc_q(d, "obs_level", *slot[o]))
    n = add("anc_" + ba_name[3:], "anchored", decision or c.decision, c.side, d, w, band=band, fixed=fixed)
    CONVERTED[n] = (ba_name, slot)
    return n


for _n in [n for n in list(CASES) if n.startswith("ba_obs_chi2_")] + ["ba_depth_fixed_behind", "ba_depth_fixed_in_front", "ba_stale_erase", "ba_stale_erase_not_excluded",
                                                                       "ba_point_leaves", "ba_point_stays", "ba_assoc_minus_1", "ba_rho_zero", "ba_rho_nonzero",
                                                                       "ba_lm_reject", "ba_lm_accept"]:
    convert(_n)
convert("ba_float_vs_double", "fx.float_vs_double")
convert("ba_float_vs_double_below_both", "fx.float_vs_double")


def anc_data(F, L=12, prior=1, comps=None, prm=None):
    """the first L points of grid(), seen exactly and in stereo by the frame and by F fixed key-frames, all at the identity"""
    X = grid()[:L].copy()
    mean, cov = mk_map(comps) if comps is not None else NOMAP
    d = dict(pose=ID7.copy(), Xw=X, obs=project(ID7, X), oct=np.zeros(L, np.int32), prior=prior, fixed_pose=np.tile(ID7, (F, 1)),
             fixed_obs=np.repeat(project(ID7, X)[:, None], F, 1), fixed_oct=np.zeros((L, F), np.int32), mean=mean, cov=cov)
    if prm:
        d["prm"] = prm
    return d


NONE = lambda L: -np.ones(L, np.int32)

# The twins of the "ba" cases whose association the call itself would not make: their point lies 1 cm (ba_assoc_0: d2 = 100) or 0.3 m
# (ba_far_from_plane: d2 = 90 000) from a 1 mm plane, outside the gate d2 <= 9, or 0.3 m from a 0.1 m blob (ba_far_from_blob: d2 = 9 (1 - 1.3e-15), ON
# the gate, where one ulp of an input decides).  ba.assoc_none: the plane 2 mm behind point 1 (d2 = 4: associated,
# the point moves towards it); the converted ba_assoc_minus_1 is the other side, gated out.  ba.nondegenerate: point 1 starts ON its
# component and every observation of it is that of a point 0.3 m deeper (ba_lambda2 = 100): off a plane it is dropped, off a blob nothing is.
_d = anc_data(1, comps=[plane(0.0, -0.25, 2.002), blob(0.0, 0.0, -50.0)])
_a = NONE(12)
_a[1] = 0
add("anc_assoc_0", "anchored", "ba.assoc_none", "associated (anchored)", _d, dict(assoc=_a, fixed_erase=fe_of(12, 1), moved_points=[1]))
# the gate itself, as track_gate_at_9 / track_gate_above_9: point 5 exactly 3 sigma from a unit-covariance component, and one ulp farther
for _n, _x, _side in (("anc_gate_at_9", 3.0, "d2 = 9.0 (anchored)"), ("anc_gate_above_9", float(np.nextafter(3.0, 4.0)), "d2 > 9.0 (anchored)")):
    _d = anc_data(1, comps=[blob(0.0, 0.25, 8.0, 1.0)])
    _d["Xw"][5] = (_x, 0.25, 8.0)
    _d["obs"][5] = _d["fixed_obs"][5, 0] = project(ID7, _d["Xw"][5])
    _a = NONE(12)
    _a[5] = 0 if _x == 3.0 else -1
    add(_n, "anchored", "ba.assoc_none", _side, _d, dict(assoc=_a, fixed_erase=fe_of(12, 1), d2_of={5: 9.0} if _x == 3.0 else {}),
        fixed=[("Xw", (5, 0)), ("Xw", (5, 1)), ("Xw", (5, 2)), ("mean", None), ("cov", None)])
for _n, _comp, _side in (("anc_far_from_plane", plane, "degenerate (anchored)"), ("anc_dragged_off_blob", blob, "not degenerate (anchored)")):
    _d = anc_data(1, comps=[_comp(0.0, -0.25, 2.0), blob(0.0, 0.0, -50.0)], prm=STR_PRM)
    _d["obs"][1] = _d["fixed_obs"][1, 0] = project(ID7, np.array([0.0, -0.25, 2.3]))
    _a = NONE(12)
    _a[1] = -1 if _comp is plane else 0
    add(_n, "anchored", "ba.nondegenerate", _side, _d, dict(assoc=_a, fixed_erase=fe_of(12, 1), moved_points=[1]))


# fx.chi2_level: the ba_thr_data scene with F = 1 ... 4: eight points, the frame and every fixed key-frame see each of them exactly, but the
# observation of point 0 from column kf, d px off in u (monocular, or stereo with u_right exact).  The exact observations hold the point, so d is
# solved per (mono, octave, F); the twin with the edge in the last column reuses it (the same problem with two key-frames exchanged).  Octave 7
# is the last entry of the sigma^2 table and the edge of the level mask.
def fx_thr_data(d, octave, mono, F=1, kf=0):
    a = anc_data(F, 8)
    a["fixed_obs"][0, kf] = sh(PR[0], d, mono=mono)
    a["fixed_oct"][0, kf] = octave
    return a


for _mono, _thr in ((True, TH_MONO), (False, TH_STEREO)):
    for _oct in (0, 2, 7):
        for _F in (1, 2, 3, 4):
            for _side, _f in (("below", 1 - REL), ("above", 1 + REL)):
                _k = "fx_chi2_%s_oct%d_F%d_%s" % ("mono" if _mono else "stereo", _oct, _F, _side)
                _d = scalar(_k, lambda o=_oct, m=_mono, F=_F, t=_thr * _f, s=1.2 ** _oct: secant(lambda d: anc_q(fx_thr_data(d, o, m, F), "obs_level", 0, 0)(numpy_ref), t, 4.0 * s, 6.0 * s))
                for _kf in sorted({0, _F - 1}):
                    _data = fx_thr_data(_d, _oct, _mono, _F, _kf)
                    add("fx_chi2_%s_oct%d_F%d_kf%d_%s" % ("mono" if _mono else "stereo", _oct, _F, _kf, _side), "anchored", "fx.chi2_level", _side, _data,
                        dict(assoc=NONE(8), fixed_erase=fe_of(8, _F, *([(0, _kf)] if _side == "above" else []))),
                        band=dict(thr=_thr, side=_side, q=anc_q(_data, "obs_level", 0, _kf)), fixed=[("fixed_obs", (0, _kf, 0))])

# fx.depth: a key-frame turned by RY7 looks away from point 0; its monocular measurement is the point's projection through the negative z, so
# chi2 is exactly 0 and the edge goes on !(zf > 0) in THAT camera alone (F = 1; the twin faces the point).  Third scene: F = 3, the
# middle key-frame looks away, the two others see every point exactly: one column of fixed_erase, and nothing moves.
for _n, _F, _kf, _pose, _side in (("fx_depth_behind", 1, 0, RY7, "behind the observer"), ("fx_depth_in_front", 1, 0, ID7, "in front of the observer"),
                                  ("fx_depth_behind_one_of_three", 3, 1, RY7, "behind one observer of three")):
    _d = anc_data(_F)
    _d["fixed_pose"][_kf] = _pose
    _d["fixed_oct"][1:, _kf] = -1
    _d["fixed_obs"][0, _kf] = sh(project(_pose, grid()[0]), mono=True)
    add(_n, "anchored", "fx.depth", _side, _d, dict(assoc=NONE(12), fixed_erase=fe_of(12, _F, *([(0, _kf)] if _pose is RY7 else [])), iters=1, outer=3, unchanged=True))

# fx.depth_own_camera: point 0 lies BEHIND the frame (its own monocular measurement is the projection through the negative z: that edge goes),
# both observers are turned by RY7 and face it, with exact observations of it alone: their edges stay.  The twin: nothing is behind anything.
_d = anc_data(2)
_d["Xw"][0] = (-0.5, -0.25, -2.0)
_d["obs"][0] = sh(project(ID7, _d["Xw"][0]), mono=True)
_d["fixed_pose"][:] = RY7
_d["fixed_oct"][1:] = -1
_d["fixed_obs"][0, :] = project(RY7, _d["Xw"][0])
add("fx_depth_own_camera_behind", "anchored", "fx.depth_own_camera", "behind the frame, in front of both observers", _d, dict(assoc=NONE(12), fixed_erase=fe_of(12, 2), iters=1, outer=3, unchanged=True))
add("fx_depth_own_camera_in_front", "anchored", "fx.depth_own_camera", "in front of all three", anc_data(2), dict(assoc=NONE(12), fixed_erase=fe_of(12, 2), iters=1, outer=3, unchanged=True))

# fx.stale_erase: the construction of ba_stale_erase (whose converted form has B in column 0 and A in column 1) with B in the LAST column
for _n, _dB, _side, _er in (("fx_stale_erase_last_column", 2.2, "erased on the stale chi2, last column", [(0, 0), (0, 1)]), ("fx_stale_erase_last_column_not_excluded", 1.0, "kept, last column", [(0, 0)])):
    _d = anc_data(2)
    _d["fixed_obs"][0, 0], _d["fixed_obs"][0, 1] = sh(PR[0], -30.0, 0, -30.0), sh(PR[0], _dB, mono=True)
    add(_n, "anchored", "fx.stale_erase", _side, _d, dict(assoc=NONE(12), fixed_erase=fe_of(12, 2, *_er)))

# fx.mono_by_uright: the observation of point 0 from column 0 is exact in u and v, its u_right 0 - 96 px from the point's.  Stereo: erased
for _n, _ur, _side in (("fx_uright_minus_0", -0.0, "stereo"), ("fx_uright_plus_0", 0.0, "stereo"), ("fx_uright_minus_denormal", -5e-324, "mono"), ("fx_uright_minus_1", -1.0, "mono")):
    _d = anc_data(2)
    _d["fixed_obs"][0, 0, 2] = _ur
    add(_n, "anchored", "fx.mono_by_uright", _side, _d, dict(assoc=NONE(12), fixed_erase=fe_of(12, 2, *([(0, 0)] if _side == "stereo" else []))), fixed=[("fixed_obs", (0, 0, 2))])


# fx.not_observed: what is marked not observed is not read.  The frame moves (the observation of point 0 from column 0 is 3 px off), and
# its outputs are those of the twin (`same_as`: data, the twin's rows and columns in this case), bit for bit
def moving(F):
    d = anc_data(F)
    d["fixed_obs"][0, 0] = sh(PR[0], 3.0)
    return d


WILD = np.array([900.0, -700.0, 5.0])
_t = moving(2)
_t["fixed_oct"][0, 1] = -1
_d = dict(_t, fixed_obs=_t["fixed_obs"].copy())
_d["fixed_obs"][0, 1] = WILD
add("fx_not_observed_edge", "anchored", "fx.not_observed", "one edge", _d, dict(assoc=NONE(12), fixed_erase=fe_of(12, 2), moved_points=[0], same_as=(_t, np.arange(12), np.arange(2))))
for _n, _pose, _side in (("fx_not_observed_keyframe", ID7, "a key-frame"), ("fx_not_observed_keyframe_turned", RY7, "a key-frame that looks away")):
    _d = moving(3)
    _d["fixed_oct"][:, 1] = -1
    _d["fixed_obs"][:, 1] = WILD
    _d["fixed_pose"][1] = _pose
    add(_n, "anchored", "fx.not_observed", _side, _d, dict(assoc=NONE(12), fixed_erase=fe_of(12, 3), moved_points=[0], same_as=(moving(2), np.arange(12), np.array([0, 2]))))
_d = moving(2)
for _k, _v in (("Xw", [[0.3, 0.1, 3.0]]), ("obs", [WILD]), ("oct", [-1]), ("fixed_obs", [[WILD, WILD]]), ("fixed_oct", [[0, 3]])):
    _d[_k] = np.concatenate([_d[_k][:5], np.array(_v, _d[_k].dtype), _d[_k][5:]])
_a = fe_of(13, 2)
add("fx_not_observed_slot", "anchored", "fx.not_observed", "a slot without a map point", _d, dict(assoc=NONE(13), fixed_erase=_a, moved_points=[0], same_as=(moving(2), np.array([0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12]), np.arange(2))))

# fx.point_keeps_fixed_edges / fx.point_leaves: the frame's own observation of point 0 is 40 px off (monocular) and excluded at :799.
#   keeps:  one fixed edge (the LAST column, 1 px off in u and u_right) stays and holds the point (`held`: it ends within 1 cm of its start, and moves)
#   leaves: every fixed edge is excluded too (40 px each, against one another) and nothing is associated: no level-0 edge, the point
#           keeps the bits of the second optimize(5) (frozen_points, by numpy_ref's instrumentation)
#   held by the map: as `leaves`, but point 0 starts 1 cm beside a tight blob, inside the gate: the GMM edge keeps it active and it ends at the centre
# each with F = 1 and F = 4 (the other columns of `keeps` are 40 px off as well), so that the test for "a fixed edge left" meets one bit and four
OFF4 = ((-40.0, 0.0, 40.0), (40.0, 40.0, -40.0), (-40.0, -40.0, -40.0), (0.0, 40.0, 40.0))


def fx_point_data(F, stays, comps=None):
    d = anc_data(F, comps=comps)
    d["obs"][0] = sh(PR[0], 40.0, mono=True)
    for j in range(F):
        d["fixed_obs"][0, j] = sh(PR[0], *OFF4[j])
    if stays:
        d["fixed_obs"][0, F - 1] = sh(PR[0], 1.0, 0.0, 1.0)
    return d


for _F in (1, 4):
    _all = [(0, j) for j in range(_F)]
    add("fx_point_keeps_one_edge_F%d" % _F, "anchored", "fx.point_keeps_fixed_edges", "one fixed edge of %d stays" % _F, fx_point_data(_F, True),
        dict(assoc=NONE(12), fixed_erase=fe_of(12, _F, *_all[:-1]), held={0: 0.01}))
    add("fx_point_leaves_F%d" % _F, "anchored", "fx.point_leaves", "no edge left, F = %d" % _F, fx_point_data(_F, False),
        dict(assoc=NONE(12), fixed_erase=fe_of(12, _F, *_all), frozen_points=[0], n_shrinks=True))
    _d = fx_point_data(_F, False, comps=[blob(-0.49, -0.25, 2.0, 0.011), blob(0.0, 0.0, -50.0)])
    _a = NONE(12)
    _a[0] = 0
    add("fx_point_held_by_map_F%d" % _F, "anchored", "fx.point_leaves", "the GMM edge keeps it, F = %d" % _F, _d,
        dict(assoc=_a, fixed_erase=fe_of(12, _F, *_all), at_mean={0: (0, True)}))


# fx.str_level / fx.str_drop: str_a_data / str_b_data with point 1 started ON its 1 mm plane (d2 = 0: inside the gate), where the "ba" cases
# start it at z = 2, 2 cm and 11 cm off.  (a): the frame and two observers exact, two observers outlying; (b): the frame and one
# observer exact, one outlying.  One scalar, the plane's offset, per side
def fx_str_data(mk, p):
    b = mk(p)
    b["points"] = b["points"].copy()
    b["points"][1, 2] = b["mean"][0][2]
    return anchored_from_ba(b)[0]


for _side, _f in (("below", 1 - REL), ("above", 1 + REL)):
    _p = scalar("fx_str_level_" + _side, lambda t=TH_STR100 * _f: secant(lambda p: anc_q(fx_str_data(str_a_data, p), "str_level", 1)(numpy_ref), t, 0.02, 0.03))
    _data = fx_str_data(str_a_data, _p)
    _a = NONE(12)
    _a[1] = 0
    add("fx_str_level_" + _side, "anchored", "fx.str_level", _side, _data, dict(assoc=_a, fixed_erase=fe_of(12, 4, (1, 2), (1, 3)), at_exact={1: (grid()[1], _side == "above")}),
        band=dict(thr=TH_STR100, side=_side, q=anc_q(_data, "str_level", 1)), fixed=[("mean", (0, 2)), ("Xw", (1, 2))])
    _p = scalar("fx_str_drop_" + _side, lambda t=TH_STR100 * _f: secant(lambda p: anc_q(fx_str_data(str_b_data, p), "str_drop", 1)(numpy_ref), t, 0.09, 0.10))
    _data = fx_str_data(str_b_data, _p)
    _a = NONE(12)
    _a[1] = -1 if _side == "above" else 0
    add("fx_str_drop_" + _side, "anchored", "fx.str_drop", _side, _data, dict(assoc=_a, fixed_erase=fe_of(12, 2, (1, 1)), at_exact={1: (grid()[1], False)}),
        band=dict(thr=TH_STR100, side=_side, q=anc_q(_data, "str_drop", 1)), fixed=[("mean", (0, 2)), ("Xw", (1, 2))])

# fx.prior_or_fixed: the ba_prior_row1 idea on the frame's own pose: its eight observations are 1 px off in u and u_right, two fixed
# observers are exact.  With the prior edge the pose moves; fixed, it keeps its bytes and the points move; without either it moves
# further than under the prior (`further_than`: against the same implementation's pose on the named case)
for _n, _pr, _fp, _side in (("fx_prior_as_prior", 1, 1, "prior edge"), ("fx_prior_as_fixed", 1, 0, "fixed"), ("fx_prior_none", 0, 1, "free")):
    _d = anc_data(2, 8, prior=_pr, prm=dict(ba_first_as_prior=_fp))
    _d["obs"] = np.stack([sh(PR[l], 1.0, 0, 1.0) for l in range(8)])
    _w = dict(assoc=NONE(8), fixed_erase=fe_of(8, 2))
    _w.update(dict(pose_bytes=True, moved_points=list(range(8))) if (_pr and not _fp) else dict(moved_pose=True))
    if not _pr:
        _w["further_than"] = "fx_prior_as_prior"
    add(_n, "anchored", "fx.prior_or_fixed", _side, _d, _w)


def pad_anchored(data, M, F, where="behind"):
    """an "anchored" case with M slots and F fixed key-frames: the added slots have octave -1 and the added key-frames (at the identity)
    observe nothing; the padding lies behind the case's rows and columns, or in front of them -> (data, rows, columns of the case)"""
    n, f = data["fixed_oct"].shape
    rows, cols = (np.arange(n), np.arange(f)) if where == "behind" else (np.arange(M - n, M), np.arange(F - f, F))
    d = dict(data, Xw=np.ones((M, 3)), obs=np.zeros((M, 3)), oct=-np.ones(M, np.int32), fixed_pose=np.tile(ID7, (F, 1)),
             fixed_obs=np.zeros((M, F, 3)), fixed_oct=-np.ones((M, F), np.int32))
    for k in ("Xw", "obs", "oct"):
        d[k][rows] = data[k]
    d["fixed_pose"][cols] = data["fixed_pose"]
    d["fixed_obs"][np.ix_(rows, cols)], d["fixed_oct"][np.ix_(rows, cols)] = data["fixed_obs"], data["fixed_oct"]
    return d, rows, cols


def unpad_anchored(o, d, rows, cols):
    """the outputs on a padded case brought back to the case's rows and columns; the padding's: assoc -1, fixed_erase 0, the point's bytes"""
    pad = np.ones(len(d["oct"]), bool)
    pad[rows] = False
    assert (o["assoc"][pad] == -1).all() and o["points"][pad].tobytes() == d["Xw"][pad].tobytes(), "a padding slot was written"
    fe = o["fixed_erase"].copy()
    fe[np.ix_(rows, cols)] = 0
    assert not fe.any(), "fixed_erase set in the padding"
    out = dict(o, assoc=o["assoc"][rows], points=o["points"][rows], d2=o["d2"][rows], fixed_erase=o["fixed_erase"][np.ix_(rows, cols)])
    return out


def check_related(c, o, other):
    """what a case declares against ANOTHER run of the same implementation (other: that run's outputs): `same_as` - the twin without the
    column or slot that is marked not observed - by the bytes; `further_than` - the pose has moved further than the named case's"""
    w = c.want
    if "same_as" in w:
        _, rows, cols = w["same_as"]
        assert o["pose"].tobytes() == other["pose"].tobytes() and o["points"][rows].tobytes() == other["points"].tobytes(), (c.name, "not the twin's bytes")
        assert np.array_equal(o["assoc"][rows], other["assoc"]) and np.array_equal(o["fixed_erase"][np.ix_(rows, cols)], other["fixed_erase"]), (c.name, "not the twin's integers")
    if "further_than" in w:
        assert np.abs(o["pose"] - c.data["pose"]).max() > np.abs(other["pose"] - c.data["pose"]).max() > 1e-6, (c.name, o["pose"], other["pose"])


def related_data(c):
    """the data of the run check_related compares with, or None"""
    return c.want["same_as"][0] if "same_as" in c.want else CASES[c.want["further_than"]].data if "further_than" in c.want else None


# ---- padding to a common launch shape ------------------------------------------------------------------------------------------------
def pad_rows(data, M):
    """a pose / track case with M slots: the rows beyond its own have octave -1 (no map point)"""
    n = len(data["oct"])
    d = dict(data)
    d["Xw"] = np.concatenate([data["Xw"], np.ones((M - n, 3))])
    d["obs"] = np.concatenate([data["obs"], np.zeros((M - n, 3))])
    d["oct"] = np.concatenate([data["oct"], -np.ones(M - n, np.int32)]).astype(np.int32)
    return d


def pad_ba(data, P, F, L):
    """a local-BA case with P free and F fixed key-frames and L points: the added key-frames (at the identity) and points have no
    observation, no prior and no association.  The fixed key-frames move up by the added free ones."""
    dP, n = P - data["P"], len(data["points"])
    d = dict(data, P=P, F=F)
    d["poses"] = np.concatenate([data["poses"][:data["P"]], np.tile(ID7, (dP, 1)), data["poses"][data["P"]:], np.tile(ID7, (F - data["F"], 1))])
    d["prior"] = np.concatenate([data["prior"], np.zeros(dP, np.uint8)])
    d["points"] = np.concatenate([data["points"], np.tile([0.0, 0.0, 2.0], (L - n, 1))])
    d["assoc"] = np.concatenate([data["assoc"], -np.ones(L - n, np.int32)]).astype(np.int32)
    d["obs_ptr"] = np.concatenate([data["obs_ptr"], np.full(L - n, data["obs_ptr"][-1], np.int32)]).astype(np.int32)
    d["obs_pose"] = np.where(data["obs_pose"] >= data["P"], data["obs_pose"] + dP, data["obs_pose"]).astype(np.int32)
    return d


def check_declared(c, o, data=None, want=None):
    """what the case declares against the outputs o of one implementation (the CPU ones, or the device's).  Integers exactly; "unchanged"
    by the bytes; the entries that need numpy_ref's instrumentation only where o carries it (o["trace"])."""
    data, w = data or c.data, want or c.want
    eq = lambda k, n=None: np.array_equal(np.asarray(o[k])[:n], np.asarray(w[k])[:n])
    tr = o.get("trace")
    if c.call == "pose":
        assert eq("outl", len(c.data["oct"])) and int(o["nin"]) == w["nin"], (c.name, o["outl"], o["nin"])
        if w.get("unchanged"):
            assert o["pose"].tobytes() == data["pose"].tobytes(), (c.name, "pose", o["pose"])
        if w.get("at_identity"):
            assert np.abs(o["pose"] - ID7).max() < 1e-6, (c.name, o["pose"])  # (the start is 1e-2 or more away)
        if tr:
            for e, f in w.get("flag_after_round0", {}).items():
                assert tr[0]["flag"][e] == f, (c.name, "flag after round 0", e)
            if "first_q" in w:  # the trials of the first outer iteration of round 0: 1 + the rejections in a row
                assert tr[0]["lm"][0]["q"][0] == w["first_q"] and tr[0]["lm"][0]["ni_max"] >= 2.0 ** w["first_q"], (c.name, tr[0]["lm"][0])
            if "q_round0" in w:
                assert tr[0]["lm"][0]["q"] == w["q_round0"], (c.name, tr[0]["lm"][0])
        return
    if c.call == "anchored":  # (o: in the case's own rows and columns - unpad_anchored brings a padded run there)
        assert eq("assoc") and eq("fixed_erase"), (c.name, o["assoc"], o["fixed_erase"])
        start = lambda l: np.abs(o["points"][l] - data["Xw"][l]).max()
        for l, v in w.get("d2_of", {}).items():
            assert o["d2"][l] == v, (c.name, "d2", o["d2"][l])
        if w.get("unchanged"):
            assert o["pose"].tobytes() == data["pose"].tobytes() and o["points"].tobytes() == data["Xw"].tobytes(), (c.name, "not the input's bytes")
        if w.get("pose_bytes"):
            assert o["pose"].tobytes() == data["pose"].tobytes(), (c.name, "a fixed pose moved", o["pose"])
        if w.get("moved_pose"):
            assert np.abs(o["pose"] - data["pose"]).max() > 1e-6, (c.name, "pose", o["pose"])
        for l in np.nonzero(data["oct"] < 0)[0]:  # a slot without a map point is no vertex
            assert o["points"][l].tobytes() == data["Xw"][l].tobytes(), (c.name, "slot", l)
        for l in w.get("moved_points", ()):
            assert start(l) > 1e-6, (c.name, "point", l)
        for l, r in w.get("held", {}).items():
            assert 1e-6 < start(l) < r, (c.name, "point", l, start(l))
        for l, (x, v) in w.get("at_exact", {}).items():
            assert (np.abs(o["points"][l] - x).max() < 1e-6) == v, (c.name, "point", l, o["points"][l])
        if w.get("at_identity"):
            assert np.abs(o["pose"] - ID7).max() < 1e-6, (c.name, o["pose"])
        for l, (a, v) in w.get("at_mean", {}).items():
            dist = np.abs(o["points"][l] - np.asarray(data["mean"])[a]).max()
            assert (dist < 1e-6) == v and (v or dist > 4e-4), (c.name, "point", l, dist)
        if tr:
            if "first_q" in w:
                assert tr["lm"][0]["q"][0] == w["first_q"] and tr["lm"][0]["ni_max"] >= 2.0 ** w["first_q"], (c.name, tr["lm"][0])
            if "n_last" in w or "n_shrinks" in w:
                assert (tr["lm"][0]["n"] > tr["lm"][-1]["n"]) == bool(w.get("n_shrinks")) and w.get("n_last", tr["lm"][-1]["n"]) == tr["lm"][-1]["n"], (c.name, [t["n"] for t in tr["lm"]])
            for l in w.get("frozen_points", ()):  # (every slot of such a case holds a point: slot l is vertex l)
                assert o["points"][l].tobytes() == tr["state_level"][1][l].tobytes(), (c.name, "point", l)
        if "outer" in w and "outer" in o:
            assert o["outer"] == w["outer"], (c.name, o["outer"])
    elif c.call == "track":
        assert eq("assoc", len(c.data["oct"])), (c.name, o["assoc"])
        for l, v in w.get("d2_of", {}).items():
            assert o["d2"][l] == v, (c.name, "d2", o["d2"][l])
        if w.get("unchanged"):
            assert o["pose"].tobytes() == data["pose"].tobytes() and o["points"].tobytes() == data["Xw"].tobytes(), (c.name, "not the input's bytes")
        for l in w.get("moved_points", ()):
            assert np.abs(o["points"][l] - data["Xw"][l]).max() > 1e-6, (c.name, "point", l)
        if w.get("at_identity"):
            assert np.abs(o["pose"] - ID7).max() < 1e-6, (c.name, o["pose"])
        for l, v in w.get("at_mean", {}).items():  # the point at the centre of the component it started nearest to (component l), or 0.5 mm or more away
            dist = np.abs(o["points"][l] - np.asarray(data["mean"])[l]).max()
            assert (dist < 1e-6) == v and (v or dist > 4e-4), (c.name, "point", l, dist)
        if tr and "first_q" in w:
            assert tr["lm"][0]["q"][0] == w["first_q"] and tr["lm"][0]["ni_max"] >= 2.0 ** w["first_q"], (c.name, tr["lm"][0])
        if "outer" in w and "outer" in o:  # the outer iterations of the three optimize() together
            assert o["outer"] == w["outer"], (c.name, o["outer"])
    else:
        nobs, L, P = len(c.data["obs_pose"]), len(c.data["points"]), c.data["P"]
        assert eq("dropped", L) and eq("erase", nobs), (c.name, o["dropped"], o["erase"])
        if w.get("unchanged"):
            assert o["poses"][:P].tobytes() == c.data["poses"][:P].tobytes() and o["points"][:L].tobytes() == c.data["points"].tobytes(), (c.name, "not the input's bytes")
        for j in w.get("unchanged_poses", ()):
            assert o["poses"][j].tobytes() == c.data["poses"][j].tobytes(), (c.name, "pose", j, o["poses"][j])
        for j in w.get("moved_poses", ()):
            assert np.abs(o["poses"][j] - c.data["poses"][j]).max() > 1e-6, (c.name, "pose", j)
        for l in w.get("moved_points", ()):
            assert np.abs(o["points"][l] - c.data["points"][l]).max() > 1e-6, (c.name, "point", l)
        for l, v in w.get("at_exact", {}).items():
            assert (np.abs(o["points"][l] - c.data["points"][l]).max() < 1e-6) == v, (c.name, "point", l, o["points"][l])
        if w.get("at_identity"):
            assert np.abs(o["poses"][0] - ID7).max() < 1e-6, (c.name, o["poses"][0])
        if tr:
            if "first_q" in w:
                assert tr["lm"][0]["q"][0] == w["first_q"] and tr["lm"][0]["ni_max"] >= 2.0 ** w["first_q"], (c.name, tr["lm"][0])
            if "n_last" in w:
                assert tr["lm"][-1]["n"] == w["n_last"] and (tr["lm"][0]["n"] > w["n_last"]) == bool(w.get("n_shrinks")), (c.name, [t["n"] for t in tr["lm"]])
            for l in w.get("frozen_points", ()):
                assert o["points"][l].tobytes() == tr["state_level"][1][l].tobytes(), (c.name, "point", l)
            for j in w.get("frozen_poses", ()):
                assert o["poses"][j].tobytes() == tr["state_level"][0][j].tobytes(), (c.name, "pose", j)
    if "iters" in w and "iters" in o:
        assert o["iters"] == w["iters"], (c.name, "iters", o["iters"])


def names(call):
    return sorted(n for n, c in CASES.items() if c.call == call)


if __name__ == "__main__":  # python -m tests.optim_cases: solve every scalar again and print the table for SOLVED
    for k, fn in SOLVERS.items():
        print('    "%s": "%s",' % (k, float(fn()).hex()))
