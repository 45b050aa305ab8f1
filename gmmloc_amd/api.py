"""Host-side mirror of the reference's interface for the hot path, over the C-ABI.

Names follow the reference (``GMM.renderView`` + ``searchCorrespondence`` ->
``GMM.search2d``, ``GMM.queryPoint``, ``optimize_current_pose`` =
``Tracking::optimizeCurrentPose`` ...).  Device buffers are torch CUDA tensors
(PyTorch-ROCm is used for memory, streams and torch.distributed only); every
function launches hand-written HIP kernels through ``libgmmloc_hip.so``.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._host import (MAP_BA_DTYPES, MAP_TABLES, MAP_VIEW_DTYPES, MAP_VIEW_POINT_KEYS, GLError, _check, _count, _map_ba_view,  # noqa: F401
                    _map_edit, _map_view, _outputs, _ptr, _tensor)

ASSOC_BRUTE = 0
ASSOC_KNN5_EUCLID = 1
ASSOC_EXHAUSTIVE = 2
ASSOC_SCREENED = 3  # the same output as ASSOC_EXHAUSTIVE, bit for bit: fp32 screen + fp64 verify of the survivors

F_MEAN, F_COV, F_COV_INV, F_DET, F_SCALE, F_AXIS, F_SQRT_INFO, F_FLAGS, F_NBS_PTR, F_NBS_IDX, F_NBS_DIST, F_HGW, F_PLANE4 = range(13)
TIMER_ASSOC, TIMER_REFINE_POSE, TIMER_BA, TIMER_BA_PREP = 0, 1, 2, 3
COUNTER_BA_REDONE, COUNTER_MATCH_ROUNDS, COUNTER_MATCH_UNITS = 0, 1, 2
COUNTER_ASSOC_SCREEN_VERIFIED, COUNTER_ASSOC_SCREEN_FALLBACK = 4, 5


@dataclass
class Camera:
    """PinholeCamera + camera::bf.  Defaults: gmmloc_ros/cfg/v1.yaml:5-17 read as float
    (config.h:38: `extern float fx, fy, cx, cy`)."""
    fx: float = float(np.float32(435.2046959714599))
    fy: float = float(np.float32(435.2046959714599))
    cx: float = float(np.float32(367.4517211914062))
    cy: float = float(np.float32(252.2008514404297))
    bf: float = float(np.float32(47.90639384423901))
    width: int = 752
    height: int = 480

    def c(self):
        return _lib.gl_camera(self.fx, self.fy, self.cx, self.cy, self.bf, self.width, self.height)


class Params:
    """Hot-path config values (config.h:31-89); defaults = cfg/v1.yaml."""

    def __init__(self, **kw):
        self._c = _lib.gl_params()
        _lib.load().gl_default_params(C.byref(self._c))
        for k, v in kw.items():
            setattr(self._c, k, v)

    def c(self):
        return self._c

    @property
    def sigma2_inv(self):
        return np.array(list(self._c.sigma2_inv), dtype=np.float32)


class Context:
    """gl_ctx_t: device + HIP stream + scratch.

    The context owns a dedicated torch stream (``ctx.stream``) and launches every kernel on
    it.  (torch's default stream is NOT ordered with kernels an external library puts on
    HIP's null stream -- measured on the MI355X box -- so the null stream is never used.)
    Every wrapper enqueues through ``call``, which orders the context stream against torch's
    current stream with events (``_enter`` / ``_exit``); under
    ``with torch.cuda.stream(ctx.stream):`` both are no-ops and calls are fully asynchronous.
    """

    def __init__(self, device=0):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        self.device = device
        with torch.cuda.device(device):
            self.stream = torch.cuda.Stream(device)
        h = C.c_void_p()
        _check(self.lib.gl_ctx_create(device, C.c_void_p(self.stream.cuda_stream), C.byref(h)))
        self.h = h

    def _enter(self):
        cur = self.torch.cuda.current_stream(self.device)
        if cur != self.stream:
            self.stream.wait_stream(cur)

    def _exit(self):
        cur = self.torch.cuda.current_stream(self.device)
        if cur != self.stream:
            cur.wait_stream(self.stream)

    def call(self, fn, *args):
        """the one enqueue: fn(ctx handle, *args) between _enter and _exit, its return code checked (GLError)"""
        self._enter()
        try:
            _check(fn(self.h, *args))
        finally:
            self._exit()

    def synchronize(self):
        _check(self.lib.gl_ctx_synchronize(self.h))

    def set_option(self, name, value):
        """gl_ctx_set_option: tuning / test knob of this context (see include/gmmloc_hip.h)."""
        _check(self.lib.gl_ctx_set_option(self.h, name.encode(), float(value)))

    def get_option(self, name):
        v = C.c_double()
        _check(self.lib.gl_ctx_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def timing(self, on):
        _check(self.lib.gl_ctx_timing_enable(self.h, 1 if on else 0))

    def timing_read(self, timer, reset=True):
        ms, n = C.c_double(), C.c_int64()
        _check(self.lib.gl_ctx_timing_read(self.h, timer, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def counter_read(self, counter=0, reset=True):
        """gl_ctx_counter_read: 0 = GL_COUNTER_BA_REDONE (frames of latency-shape launches redone by the follow-up kernel),
        1 / 2 = GL_COUNTER_MATCH_ROUNDS / _UNITS (rounds of the matchers' owner fixed point, and the frames / pairs they ran on),
        4 / 5 = GL_COUNTER_ASSOC_SCREEN_VERIFIED / _FALLBACK (pairs the screened sweep re-evaluated in fp64, and points it sent
        through the full fp64 sweep)."""
        v = C.c_int64(0)
        _check(self.lib.gl_ctx_counter_read(self.h, counter, C.byref(v), 1 if reset else 0))
        return v.value

    def set_stats_buffer(self, trials, iters=None):
        """Register (or clear with None) an int32 CUDA tensor that receives per-frame LM trial counts; `iters` (same size,
        optional) receives the outer Levenberg iterations of the per-frame refine."""
        self._stats = (trials, iters)
        n = trials.numel() if trials is not None else 0
        assert iters is None or iters.numel() >= n
        _check(self.lib.gl_ctx_set_stats_buffers(self.h, _ptr(trials), _ptr(iters), n))

    def set_edge_stats_buffer(self, edges):
        """Register (or clear with None) an int32 CUDA tensor (n, 2): per frame of the on-chip refine the level-0 reprojection edges
        summed over its Levenberg trials / over its outer iterations (gl_ctx_set_edge_stats_buffer)."""
        self._edge_stats = edges
        n = edges.shape[0] if edges is not None else 0
        assert edges is None or (edges.dim() == 2 and edges.shape[1] == 2 and edges.is_contiguous())
        _check(self.lib.gl_ctx_set_edge_stats_buffer(self.h, _ptr(edges), n))

    def close(self):
        if getattr(self, "h", None):
            self.lib.gl_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GMM:
    """gmmloc::GMM (gaussian_mixture.h:98-170) on the GPU."""

    def __init__(self, ctx, mean, cov, params=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.params = params or Params()
        mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1, 3)
        cov = np.ascontiguousarray(cov, dtype=np.float64).reshape(-1, 9)
        assert mean.shape[0] == cov.shape[0]
        h = C.c_void_p()
        _check(self.lib.gl_gmm_create(ctx.h, mean.ctypes.data, cov.ctypes.data, mean.shape[0],
                                      C.byref(self.params.c()), C.byref(h)))
        self.h = h

    @classmethod
    def load(cls, ctx, path, params=None):
        """GMMUtility::loadGMMModel (gmm_utils.cpp:9-67)."""
        self = cls.__new__(cls)
        self.ctx, self.lib = ctx, ctx.lib
        self.params = params or Params()
        h = C.c_void_p()
        _check(self.lib.gl_gmm_load_file(ctx.h, str(path).encode(), C.byref(self.params.c()), C.byref(h)))
        self.h = h
        return self

    def save(self, path):
        _check(self.lib.gl_gmm_save_file(self.h, str(path).encode()))

    def countComponents(self):
        return self.lib.gl_gmm_count(self.h)

    K = property(countComponents)

    def get(self, field):
        K = self.K
        nnz = self.lib.gl_gmm_nbs_count(self.h)
        shape, dt = {
            F_MEAN: ((K, 3), np.float64), F_COV: ((K, 9), np.float64), F_COV_INV: ((K, 9), np.float64),
            F_DET: ((K,), np.float64), F_SCALE: ((K, 3), np.float64), F_AXIS: ((K, 9), np.float64),
            F_SQRT_INFO: ((K, 9), np.float64), F_FLAGS: ((K,), np.uint8), F_NBS_PTR: ((K + 1,), np.int32),
            F_NBS_IDX: ((nnz,), np.int32), F_NBS_DIST: ((nnz,), np.float64), F_HGW: ((K, 6), np.float64),
            F_PLANE4: ((K, 4), np.float64)}[field]
        out = np.zeros(shape, dtype=dt)
        _check(self.lib.gl_gmm_get(self.h, field, out.ctypes.data, out.nbytes))
        return out

    # ---- association ----------------------------------------------------------
    def associate3d(self, pts, mode=ASSOC_BRUTE, want_d2=True):
        """pts: (N,3) float64 CUDA tensor -> (idx int32 (N,), d2 float64 (N,))."""
        import torch
        N = pts.shape[0]
        idx = torch.empty(N, dtype=torch.int32, device=pts.device)
        d2 = torch.empty(N, dtype=torch.float64, device=pts.device) if want_d2 else None
        self.ctx.call(self.lib.gl_associate3d, self.h, _ptr(pts), N, mode, _ptr(idx), _ptr(d2))
        return idx, d2

    def index_info(self):
        """Cell index behind ASSOC_BRUTE: dict(enabled, cell, dims, entries, always, t_resolve)."""
        import ctypes as C
        info = (C.c_double * 8)()
        _check(self.lib.gl_gmm_index_info(self.h, info))
        b = (C.c_double * 3)()
        _check(self.lib.gl_gmm_index_bytes(self.h, b))
        return {"enabled": bool(info[0]), "cell": info[1], "dims": (int(info[2]), int(info[3]), int(info[4])),
                "entries": int(info[5]), "always": int(info[6]), "t_resolve": info[7],
                "bytes": {"cell_pointers": int(b[0]), "lists": int(b[1]), "packed_cells": int(b[2])}}

    def index_work(self, pts):
        """Number of (point, component) evaluations the cell index performs for these points."""
        import torch
        out = torch.zeros(1, dtype=torch.int64, device=pts.device)
        self.ctx.call(self.lib.gl_assoc_index_work, self.h, _ptr(pts), pts.shape[0], _ptr(out))
        return int(out.item())

    def knn3d(self, pts, k=5):
        import torch
        N = pts.shape[0]
        idx = torch.empty((N, k), dtype=torch.int32, device=pts.device)
        dist = torch.empty((N, k), dtype=torch.float64, device=pts.device)
        self.ctx.call(self.lib.gl_knn3d, self.h, _ptr(pts), N, k, _ptr(idx), _ptr(dist))
        return idx, dist

    def queryPoint(self, pts):
        """GMM::queryPoint (gaussian_mixture.cpp:545-576), batched."""
        return self.associate3d(pts, ASSOC_KNN5_EUCLID)[0]

    def close(self):
        if getattr(self, "h", None):
            self.lib.gl_gmm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def optimize_current_pose(ctx, cam, prm, pose, Xw, obs, octave, outlier=None):
    """Tracking::optimizeCurrentPose (tracking_opt.cpp:21-217) for B frames.
    pose (B,7) in/out, Xw (B,M,3), obs (B,M,3), octave (B,M) int32 (<0: no map point); outlier (B,M) uint8
    in/out (is_outlier_: rewritten where a map point exists, untouched elsewhere; default: zeros).
    Returns (outlier uint8 (B,M), ninlier int32 (B,))."""
    import torch
    B, M = octave.shape
    if outlier is None:
        outlier = torch.zeros((B, M), dtype=torch.uint8, device=pose.device)
    nin = torch.zeros(B, dtype=torch.int32, device=pose.device)
    ctx.call(ctx.lib.gl_optimize_current_pose, C.byref(cam.c()), C.byref(prm.c()), B, M, _ptr(pose), _ptr(Xw), _ptr(obs), _ptr(octave), _ptr(outlier),
             _ptr(nin))
    return outlier, nin


def track_frames(ctx, gmm, cam, prm, pose, Xw, obs, octave, want_d2=True):
    """North-star per-frame path (gl_track_frames): exhaustive Mahalanobis association of the
    M map points of each of the B frames against the K Gaussians + structure-constrained
    refinement (jointOptimization with one free pose).  pose (B,7) and Xw (B,M,3) are updated
    in place.  Returns (assoc int32 (B,M), d2 float64 (B,M) or None)."""
    import torch
    B, M = octave.shape
    assoc = torch.empty((B, M), dtype=torch.int32, device=pose.device)
    d2 = torch.empty((B, M), dtype=torch.float64, device=pose.device) if want_d2 else None
    ctx.call(ctx.lib.gl_track_frames, gmm.h, C.byref(cam.c()), C.byref(prm.c()), B, M, _ptr(pose), _ptr(Xw), _ptr(obs), _ptr(octave), _ptr(assoc),
             _ptr(d2))
    return assoc, d2


def track_frames_anchored(ctx, gmm, cam, prm, pose, Xw, obs, octave, prior=None, fixed_pose=None, fixed_obs=None,
                          fixed_oct=None, want_d2=True, want_erase=False):
    """gl_track_frames_anchored: the per-frame path with the reference's gauge anchors (localization_opt.cpp:491-516,
    556-581).  prior (B,) uint8 or None: EdgeSE3QuatPrior on the input pose (or the pose fixed when
    prm.ba_first_as_prior == 0); fixed_pose (B,F,7), fixed_obs (B,M,F,3), fixed_oct (B,M,F) int32 (<0: not observed):
    F fixed observer key-frames.  pose and Xw are updated in place.
    Returns (assoc int32 (B,M), d2 or None, fixed_erase uint8 (B,M,F) or None)."""
    import torch
    B, M = octave.shape
    F = 0 if fixed_pose is None else fixed_pose.shape[1]
    assoc = torch.empty((B, M), dtype=torch.int32, device=pose.device)
    d2 = torch.empty((B, M), dtype=torch.float64, device=pose.device) if want_d2 else None
    erase = torch.zeros((B, M, F), dtype=torch.uint8, device=pose.device) if (want_erase and F) else None
    an = _lib.gl_track_anchor(_ptr(prior), F, _ptr(fixed_pose), _ptr(fixed_obs), _ptr(fixed_oct), _ptr(erase))
    ctx.call(ctx.lib.gl_track_frames_anchored, gmm.h, C.byref(cam.c()), C.byref(prm.c()), B, M, _ptr(pose), _ptr(Xw), _ptr(obs), _ptr(octave),
             _ptr(assoc), _ptr(d2), C.byref(an))
    return assoc, d2, erase


class HostFramePath:
    """The frame-at-a-time caller with HOST buffers in and out - gl_track_frame_host, what
    include/gmmloc_hip/gmm_adapter.hpp::trackFrame does for the reference host (tracking.cpp calls the path once per
    frame): the context's page-locked staging buffer and its device mirror, one enqueued transfer each way and ONE
    synchronize per frame."""

    def __init__(self, ctx, gmm, cam, prm, max_points=0):
        self.ctx, self.gmm, self.cam, self.prm = ctx, gmm, cam.c(), prm.c()

    @staticmethod
    def _arr(a, dtype, shape, name, writable=False):
        # the C entry point reads raw host memory: a float32 Xw or an int64 octave would be read out of bounds
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.shape == shape
                and (a.flags.writeable or not writable)):
            raise TypeError("HostFramePath: %s must be a C-contiguous %s array of shape %s%s"
                            % (name, np.dtype(dtype).name, shape, " (writable: updated in place)" if writable else ""))
        return a

    def track_frame(self, pose, Xw, obs, octave, anchored=False):
        """pose (7,), Xw (M,3) float64 are updated in place; obs (M,3) float64, octave (M,) int32; returns assoc (M,) int32.
        anchored: with the prior edge on the input pose (gl_track_frame_host_anchored)."""
        M = octave.shape[0]
        self._arr(pose, np.float64, (7,), "pose", True)
        self._arr(Xw, np.float64, (M, 3), "Xw", True)
        self._arr(obs, np.float64, (M, 3), "obs")
        self._arr(octave, np.int32, (M,), "octave")
        assoc = np.empty(M, np.int32)
        fn = self.ctx.lib.gl_track_frame_host_anchored if anchored else self.ctx.lib.gl_track_frame_host
        _check(fn(self.ctx.h, self.gmm.h, C.byref(self.cam), C.byref(self.prm), M, pose.ctypes.data,
                  Xw.ctypes.data, obs.ctypes.data, octave.ctypes.data, assoc.ctypes.data))
        return assoc

    def close(self):
        pass


def read_gmm_file(path):
    """Host-only .gmm reader (gl_gmm_file_read) -> (mean (K,3), cov (K,9))."""
    lib = _lib.load()
    K = C.c_int32()
    _check(lib.gl_gmm_file_read(str(path).encode(), None, None, 0, C.byref(K)))
    mean, cov = np.zeros((K.value, 3)), np.zeros((K.value, 9))
    _check(lib.gl_gmm_file_read(str(path).encode(), mean.ctypes.data, cov.ctypes.data, K.value, C.byref(K)))
    return mean, cov


def write_gmm_file(path, mean, cov, flags):
    lib = _lib.load()
    mean = np.ascontiguousarray(mean, np.float64)
    cov = np.ascontiguousarray(cov, np.float64)
    flags = np.ascontiguousarray(flags, np.uint8)
    _check(lib.gl_gmm_file_write(str(path).encode(), mean.ctypes.data, cov.ctypes.data, flags.ctypes.data,
                                 mean.shape[0]))


def _gmm_search2d(self, cam, pose, uv, nfeat=None, k=5, view_cap=0):
    """GMMLoc::associateMapElements = GMM::renderView + GMM::searchCorrespondence for B key-frames.
    pose (B,7), uv (B,N,2) -> (cand int32 (B,N,k), ncand int32 (B,N), view_ids (B,view_cap) | None,
    nview (B,) | None)."""
    import torch
    B, N = uv.shape[0], uv.shape[1]
    cand = torch.empty((B, N, k), dtype=torch.int32, device=uv.device)
    ncand = torch.empty((B, N), dtype=torch.int32, device=uv.device)
    vids = torch.empty((B, view_cap), dtype=torch.int32, device=uv.device) if view_cap else None
    nview = torch.empty(B, dtype=torch.int32, device=uv.device) if view_cap else None
    self.ctx.call(self.lib.gl_search2d, self.h, C.byref(cam.c()), B, _ptr(pose), N, _ptr(uv), _ptr(nfeat), k, _ptr(cand), _ptr(ncand), view_cap,
                  _ptr(vids), _ptr(nview))
    return cand, ncand, vids, nview


GMM.search2d = _gmm_search2d


def optimize_point(ctx, gmm, cam, prm, pts, uvr, octave, pose, comp, proj_z2):
    """GMMLoc::optimizePoint (gmmloc_opt.cpp:260-342), N problems -> (res, chi2_proj, chi2_str, pt_est)."""
    import torch
    N = pts.shape[0]
    dev = pts.device
    res = torch.empty(N, dtype=torch.uint8, device=dev)
    c2p = torch.empty(N, dtype=torch.float64, device=dev)
    c2s = torch.empty(N, dtype=torch.float64, device=dev)
    est = torch.empty((N, 3), dtype=torch.float64, device=dev)
    ctx.call(ctx.lib.gl_optimize_point, gmm.h, C.byref(cam.c()), C.byref(prm.c()), N, _ptr(pts), _ptr(uvr), _ptr(octave), _ptr(pose), _ptr(comp),
             _ptr(proj_z2), _ptr(res), _ptr(c2p), _ptr(c2s), _ptr(est))
    return res, c2p, c2s, est


def check_map_association(ctx, gmm, cam, prm, pose, pts, uvr, octave, cand, ncand):
    """GMMLoc::checkMapAssociation (gmmloc_opt.cpp:156-258): pose (B,7), pts (B,N,3) in/out, uvr (B,N,3),
    octave (B,N), cand (B,N,k), ncand (B,N) -> out_comp (B,N)."""
    import torch
    B, N, k = cand.shape
    out = torch.empty((B, N), dtype=torch.int32, device=pts.device)
    ctx.call(ctx.lib.gl_check_map_association, gmm.h, C.byref(cam.c()), C.byref(prm.c()), B, N, _ptr(pose), _ptr(pts), _ptr(uvr), _ptr(octave),
             _ptr(cand), _ptr(ncand), k, _ptr(out))
    return out


def optimize_triangulation(ctx, gmm, cam, prm, x3d, pose1, uvr1, oct1, pose2, uvr2, oct2, cand1, n1, cand2, n2):
    """Localization::optimizeTriangulationVec (localization_opt.cpp:27-204), N problems; x3d in/out."""
    import torch
    N, k = cand1.shape
    out = torch.empty(N, dtype=torch.int32, device=x3d.device)
    ctx.call(ctx.lib.gl_optimize_triangulation, gmm.h, C.byref(cam.c()), C.byref(prm.c()), N, _ptr(x3d), _ptr(pose1), _ptr(uvr1), _ptr(oct1),
             _ptr(pose2), _ptr(uvr2), _ptr(oct2), _ptr(cand1), _ptr(n1), _ptr(cand2), _ptr(n2), k, _ptr(out))
    return out


def joint_optimization(ctx, gmm, cam, prm, P, F, poses, prior, points, assoc, obs_ptr, obs_pose, obs_uvr, obs_oct, stop_flag=None):
    """Localization::jointOptimization (localization_opt.cpp:456-925) on B flat problems of one shape.
    poses (B,P+F,7) and points (B,L,3) are updated in place.  stop_flag: int32 tensor of one element (device or
    pinned host memory) = the reference's pbStopFlag (gl_joint_optimization_stoppable: > 0 stop, < 0 iteration budget).
    Returns (assoc_dropped uint8 (B,L), obs_erase uint8 (B,NOBS), iters int32 (B,))."""
    import torch
    B, L = points.shape[0], points.shape[1]
    NOBS = obs_pose.shape[1]
    dev = points.device
    dropped = torch.zeros((B, L), dtype=torch.uint8, device=dev)
    erase = torch.zeros((B, NOBS), dtype=torch.uint8, device=dev)
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    args = [gmm.h, C.byref(cam.c()), C.byref(prm.c()), B, P, F, L, NOBS, _ptr(poses), _ptr(prior), _ptr(points), _ptr(assoc), _ptr(obs_ptr),
            _ptr(obs_pose), _ptr(obs_uvr), _ptr(obs_oct), _ptr(dropped), _ptr(erase), _ptr(iters)]
    if stop_flag is None:
        ctx.call(ctx.lib.gl_joint_optimization, *args)
    else:
        ctx.call(ctx.lib.gl_joint_optimization_stoppable, *args, _ptr(stop_flag))
    return dropped, erase, iters


def search_by_projection(ctx, cam, feat_uv, feat_ur, feat_oct, feat_desc, feat_taken, mp_uvr, mp_level, mp_viewcos,
                         mp_valid, mp_desc, th=3.0, nn_ratio=0.8, scale_factor=1.2):
    """ORBmatcher::searchByProjection (orb_matcher.cpp:27-110) for B frames.  feat_* (B,NF,...), mp_* (B,NP,...)
    device tensors -> (feat_match int32 (B,NF), nmatches int32 (B,))."""
    import torch
    B, NF = feat_oct.shape
    NP = mp_level.shape[1]
    match = torch.empty((B, NF), dtype=torch.int32, device=feat_oct.device)
    nm = torch.empty(B, dtype=torch.int32, device=feat_oct.device)
    ctx.call(ctx.lib.gl_search_by_projection, C.byref(cam.c()), float(scale_factor), B, NF, NP, _ptr(feat_uv), _ptr(feat_ur), _ptr(feat_oct),
             _ptr(feat_desc), _ptr(feat_taken), _ptr(mp_uvr), _ptr(mp_level), _ptr(mp_viewcos), _ptr(mp_valid), _ptr(mp_desc), float(th),
             float(nn_ratio), _ptr(match), _ptr(nm))
    return match, nm


def search_local_points(ctx, cam, feat_uv, feat_ur, feat_oct, feat_desc, feat_taken, pose_cw, t_wc, mp_pos, mp_normal, mp_max_dist,
                        mp_min_dist, mp_cand, mp_desc, th=3.0, nn_ratio=0.8, scale_factor=1.2):
    """Tracking::searchLocalPoints (tracking.cpp:213-270), the device part in one call: project_map_points, then
    search_by_projection on its outputs -> (feat_match int32 (B,NF), nmatches int32 (B,), inview u8 (B,NP))."""
    import torch
    B, NF = feat_oct.shape
    NP = mp_cand.shape[1]
    dev = feat_oct.device
    match = torch.empty((B, NF), dtype=torch.int32, device=dev)
    nm = torch.empty(B, dtype=torch.int32, device=dev)
    inview = torch.empty((B, NP), dtype=torch.uint8, device=dev)
    ctx.call(ctx.lib.gl_search_local_points, C.byref(cam.c()), float(scale_factor), B, NF, NP, _ptr(feat_uv), _ptr(feat_ur), _ptr(feat_oct),
             _ptr(feat_desc), _ptr(feat_taken), _ptr(pose_cw), _ptr(t_wc), _ptr(mp_pos), _ptr(mp_normal), _ptr(mp_max_dist), _ptr(mp_min_dist),
             _ptr(mp_cand), _ptr(mp_desc), float(th), float(nn_ratio), _ptr(match), _ptr(nm), _ptr(inview))
    return match, nm, inview


CHAIN_FIELDS = ("feat_uv", "feat_ur", "feat_oct", "feat_angle", "feat_desc", "feat_taken", "pose_lw", "last_pt", "last_valid", "last_oct",
                "last_angle", "last_desc", "last_to_local", "mp_pos", "mp_normal", "mp_max_dist", "mp_min_dist", "mp_cand", "mp_desc",
                "pose_cw", "pose_mm", "match_last", "match_local", "outlier", "counts", "inview")
CHAIN_DTYPES = {"feat_uv": "float64", "feat_ur": "float32", "feat_oct": "int32", "feat_angle": "float32", "feat_desc": "uint8",
                "feat_taken": "uint8", "pose_lw": "float64", "last_pt": "float64", "last_valid": "uint8", "last_oct": "int32",
                "last_angle": "float32", "last_desc": "uint8", "last_to_local": "int32", "mp_pos": "float64", "mp_normal": "float64",
                "mp_max_dist": "float32", "mp_min_dist": "float32", "mp_cand": "uint8", "mp_desc": "uint8", "pose_cw": "float64"}


# round 6: optional inputs (a key absent from `a` = NULL).  last_observed: countObservations() > 0 of the last frame's map points; the
# kf_* / feat_node_* buffers switch the trackKeyFrame fallback on.
CHAIN_OPT_DTYPES = {"last_observed": "uint8", "kf_angle": "float32", "kf_desc": "uint8", "kf_has_mp": "uint8", "kf_nnode": "int32",
                    "kf_node_id": "int32", "kf_node_ptr": "int32", "kf_node_idx": "int32", "kf_pt": "float64", "kf_to_local": "int32",
                    "feat_nnode": "int32", "feat_node_id": "int32", "feat_node_ptr": "int32", "feat_node_idx": "int32"}
CHAIN_FIELDS2A = ("last_observed", "drop_src", "counts2")
CHAIN_FIELDS2B = ("kf_angle", "kf_desc", "kf_has_mp", "kf_nnode", "kf_node_id", "kf_node_ptr", "kf_node_idx", "kf_pt", "kf_to_local",
                  "feat_nnode", "feat_node_id", "feat_node_ptr", "feat_node_idx", "match_kf", "drop_kf")


class _ChainIO(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in CHAIN_FIELDS] + [(k, C.c_void_p) for k in CHAIN_FIELDS2A] +
                [("NK", C.c_int32), ("NNK", C.c_int32), ("NNF", C.c_int32), ("reserved_", C.c_int32)] + [(k, C.c_void_p) for k in CHAIN_FIELDS2B])


def _chain_io(a, out):
    import torch
    for k, dt in CHAIN_DTYPES.items():
        t = a[k]
        assert t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch." + dt, (k, t.dtype, t.is_contiguous())
    for k, dt in CHAIN_OPT_DTYPES.items():
        if k in a and a[k] is not None:
            t = a[k]
            assert t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch." + dt, (k, t.dtype, t.is_contiguous())
    io = _ChainIO()
    for k in CHAIN_FIELDS + CHAIN_FIELDS2A + CHAIN_FIELDS2B:
        t = out["pose"] if k == "pose_cw" else (out[k] if k in out else a.get(k))
        setattr(io, k, _ptr(t) if t is not None else None)
    if a.get("kf_desc") is not None:
        io.NK, io.NNK, io.NNF = a["kf_desc"].shape[1], a["kf_node_id"].shape[1], a["feat_node_id"].shape[1]
    return io


def _chain_out(a, front_only=False, NP=None):
    import torch
    B, NF = a["feat_oct"].shape
    NP = a["mp_cand"].shape[1] if NP is None else NP
    dev = a["feat_oct"].device
    i32 = lambda *sh: torch.full(sh, -1, dtype=torch.int32, device=dev)
    out = dict(pose=a["pose_cw"].clone(), pose_mm=torch.empty((B, 7), dtype=torch.float64, device=dev), match_last=i32(B, NF),
               match_local=i32(B, NF), outlier=torch.zeros((B, NF), dtype=torch.uint8, device=dev),
               counts=torch.zeros((B, 4), dtype=torch.int32, device=dev), inview=torch.zeros((B, NP), dtype=torch.uint8, device=dev),
               drop_src=i32(B, NF), counts2=torch.zeros((B, 4), dtype=torch.int32, device=dev))
    if a.get("kf_desc") is not None:
        out["match_kf"] = i32(B, NF)
        out["drop_kf"] = i32(B, NF)
    return out


def track_frame_chain(ctx, cam, prm, a, th_mm=7.0, th_local=3.0, nn_ratio=0.8, mono=False, scale_factor=1.2, out=None):
    """gl_track_frame_chain: trackWithMotionModel (-> trackKeyFrame where it fails, if `a` holds the key-frame buffers) ->
    searchLocalPoints -> trackLocalMap for B frames, device resident.  `a`: dict of CUDA tensors with the input keys of CHAIN_DTYPES
    (+ optionally those of CHAIN_OPT_DTYPES); pose_cw (B,7): the motion-model prediction, NOT modified - the result comes back as a
    new tensor.  Returns dict(pose, pose_mm, match_last, match_local, outlier, counts (B,4), inview, drop_src, counts2 (B,4)
    [, match_kf, drop_kf]).  `out`: the dict of an earlier call, to be used again (a host that tracks frame after frame keeps its buffers:
    0.05 ms of allocations less per call); its pose is reset to a["pose_cw"] first."""
    B, NF = a["feat_oct"].shape
    NL, NP = a["last_oct"].shape[1], a["mp_cand"].shape[1]
    if out is None:
        out = _chain_out(a)
    else:
        out["pose"].copy_(a["pose_cw"])
    io = _chain_io(a, out)
    ctx.call(ctx.lib.gl_track_frame_chain, C.byref(cam.c()), C.byref(prm.c()), float(scale_factor), B, NF, NL, NP, C.byref(io), float(th_mm),
             float(th_local), float(nn_ratio), int(bool(mono)))
    return out


def track_frame_chain_front(ctx, cam, prm, a, th_mm=7.0, mono=False, scale_factor=1.2):
    """gl_track_frame_chain_front: stages 1, 2 (and the trackKeyFrame fallback) of the chain.  Returns the same dict as
    track_frame_chain (pose = the pose after stage 2 / 2b; match_local / inview / counts[2:] untouched); hand it to
    track_frame_chain_back together with the local map Tracking::updateLocalMap made from it."""
    B, NF = a["feat_oct"].shape
    NL, NP = a["last_oct"].shape[1], a["mp_cand"].shape[1]
    out = _chain_out(a)
    io = _chain_io(a, out)
    ctx.call(ctx.lib.gl_track_frame_chain_front, C.byref(cam.c()), C.byref(prm.c()), float(scale_factor), B, NF, NL, NP, C.byref(io), float(th_mm),
             int(bool(mono)))
    return out


def track_frame_chain_back(ctx, cam, prm, a, out, th_local=3.0, nn_ratio=0.8, scale_factor=1.2):
    """gl_track_frame_chain_back: stages 3, 4 on the associations `out` (of track_frame_chain_front) and the local map in `a`
    (mp_*, last_to_local, kf_to_local: indices into THIS local map).  `out` is updated in place and returned."""
    B, NF = a["feat_oct"].shape
    NL, NP = a["last_oct"].shape[1], a["mp_cand"].shape[1]
    import torch
    if out["inview"].shape[1] != NP:
        out["inview"] = torch.zeros((B, NP), dtype=torch.uint8, device=a["feat_oct"].device)
    io = _chain_io(a, out)
    ctx.call(ctx.lib.gl_track_frame_chain_back, C.byref(cam.c()), C.byref(prm.c()), float(scale_factor), B, NF, NL, NP, C.byref(io), float(th_local),
             float(nn_ratio))
    return out


# The whole map as device arrays (gl_map_view, gl_map_ba_view): _host.MAP_TABLES and what is derived from it
LOCAL_MAP_STATUS_KEPT, LOCAL_MAP_STATUS_MP_TRUNCATED, LOCAL_MAP_STATUS_KF_TRUNCATED = 1, 2, 4


def local_map_lists(B, KFcap, NPcap, NKF=None, device="cuda"):
    """The in/out lists of update_local_map / track_frame_chain_map for B frames, empty (a tracker keeps them from frame to frame):
    dict(local_kf (B,KFcap), n_local_kf (B,), local_mp (B,NPcap), n_local_mp (B,), ref_kf (B,) = -1, status (B,)[, kf_count (B,NKF)])."""
    import torch
    z = lambda *sh: torch.zeros(sh, dtype=torch.int32, device=device)
    lists = dict(local_kf=torch.full((B, KFcap), -1, dtype=torch.int32, device=device), n_local_kf=z(B),
                 local_mp=torch.full((B, NPcap), -1, dtype=torch.int32, device=device), n_local_mp=z(B),
                 ref_kf=torch.full((B,), -1, dtype=torch.int32, device=device), status=z(B))
    if NKF is not None:
        lists["kf_count"] = z(B, NKF)
    return lists


def _check_lists(lists, B, NKF, dev):
    for k in lists:
        assert k in ("local_kf", "n_local_kf", "local_mp", "n_local_mp", "ref_kf", "status", "kf_count"), "lists[%r]: unknown key" % k
    _tensor("lists['local_kf']", lists.get("local_kf"), "int32", (B, None), dev)
    _tensor("lists['local_mp']", lists.get("local_mp"), "int32", (B, None), dev)
    for k in ("n_local_kf", "n_local_mp", "ref_kf", "status"):
        _tensor("lists[%r]" % k, lists.get(k), "int32", (B,), dev)
    if lists.get("kf_count") is not None:
        _tensor("lists['kf_count']", lists["kf_count"], "int32", (B, NKF), dev)
    KFcap, NPcap = lists["local_kf"].shape[1], lists["local_mp"].shape[1]
    return KFcap, NPcap


def update_local_map(ctx, map, feat_mp, lists):
    """gl_update_local_map: Tracking::updateLocalMap (tracking.cpp:119-207) for B frames on the device (rules, reproduced quirks and
    the canonical order: gmmloc_hip.h).  `map`: dict of CUDA tensors, the whole map - obs_ptr (NMP+1,) / obs_kf (NOBS,) i32 (the CSR of
    update_map_points), kf_mp (NKF,NFK) i32 (a key-frame's mappoints_ as map-point rows, -1 null), optionally mp_valid (NMP,) /
    kf_valid (NKF,) u8.  feat_mp (B,NF) i32: the map-point row each feature holds, -1 none - IN/OUT (an invalid point's entry becomes
    -1).  `lists`: the dict of local_map_lists, IN/OUT (a frame with an empty counter keeps what it holds); returned."""
    v, dev = _map_view(map, False)
    _tensor("feat_mp", feat_mp, "int32", (None, None), dev)
    B, NF = feat_mp.shape
    KFcap, NPcap = _check_lists(lists, B, v.NKF, dev)
    ctx.call(ctx.lib.gl_update_local_map, C.byref(v), B, NF, KFcap, NPcap, _ptr(feat_mp), _ptr(lists["local_kf"]), _ptr(lists["n_local_kf"]),
             _ptr(lists["local_mp"]), _ptr(lists["n_local_mp"]), _ptr(lists["ref_kf"]), _ptr(lists.get("kf_count")), _ptr(lists["status"]))
    return lists


CHAIN_MAP_IGNORED = ("mp_pos", "mp_normal", "mp_max_dist", "mp_min_dist", "mp_cand", "mp_desc", "last_to_local", "kf_to_local")


def track_frame_chain_map(ctx, cam, prm, a, map, lm, th_mm=7.0, th_local=3.0, nn_ratio=0.8, mono=False, scale_factor=1.2):
    """gl_track_frame_chain_map: the tracked frame in Tracking::track's own sequence as ONE call - stages 1, 2, 2b, updateLocalMap on
    the device, stages 3, 4 on the local map it made.  `a`: the inputs of track_frame_chain WITHOUT the local map (the keys of
    CHAIN_MAP_IGNORED are not read; absent is fine); `map`: the whole map (update_local_map's keys + mp_pos (NMP,3) f64, mp_normal
    (NMP,3) f64, mp_max_dist / mp_min_dist (NMP,) f32, mp_desc (NMP,32) u8); `lm`: dict(last_mp (B,NL) i32, [kf_feat_mp (B,NK) i32 with
    the fallback,] + the lists of local_map_lists, IN/OUT).  Returns the dict of track_frame_chain (match_local indexes
    lm['local_mp']; inview is (B,NPcap)) + feat_mp (B,NF)."""
    import torch
    dev = _tensor("a['feat_oct']", a.get("feat_oct"), "int32", (None, None), None).device
    B, NF = a["feat_oct"].shape
    _tensor("a['last_oct']", a.get("last_oct"), "int32", (B, None), dev)
    NL = a["last_oct"].shape[1]
    fbk = a.get("kf_desc") is not None
    NK = a["kf_desc"].shape[1] if fbk else 0
    shapes = {"feat_uv": (B, NF, 2), "feat_ur": (B, NF), "feat_oct": (B, NF), "feat_angle": (B, NF), "feat_desc": (B, NF, 32), "feat_taken": (B, NF),
              "pose_lw": (B, 7), "last_pt": (B, NL, 3), "last_valid": (B, NL), "last_oct": (B, NL), "last_angle": (B, NL), "last_desc": (B, NL, 32),
              "pose_cw": (B, 7), "last_observed": (B, NL), "kf_angle": (B, NK), "kf_desc": (B, NK, 32), "kf_has_mp": (B, NK), "kf_nnode": (B,),
              "kf_node_id": (B, None), "kf_node_ptr": (B, None), "kf_node_idx": (B, NK), "kf_pt": (B, NK, 3), "feat_nnode": (B,),
              "feat_node_id": (B, None), "feat_node_ptr": (B, None), "feat_node_idx": (B, NF)}
    for k, dt in CHAIN_DTYPES.items():
        if k not in CHAIN_MAP_IGNORED:
            _tensor("a[%r]" % k, a.get(k), dt, shapes[k], dev)
    for k, dt in CHAIN_OPT_DTYPES.items():
        if k in CHAIN_MAP_IGNORED:
            continue
        if k == "last_observed":
            if a.get(k) is not None:
                _tensor("a[%r]" % k, a[k], dt, shapes[k], dev)
        elif fbk:
            _tensor("a[%r]" % k, a.get(k), dt, shapes[k], dev)
        else:
            assert a.get(k) is None, "a[%r] without a['kf_desc'] (the fallback needs all of its buffers)" % k
    if fbk:
        assert a["kf_node_ptr"].shape[1] == a["kf_node_id"].shape[1] + 1 and a["feat_node_ptr"].shape[1] == a["feat_node_id"].shape[1] + 1, \
            "node_ptr needs one entry more than node_id"
    v, mdev = _map_view(map, True)
    assert mdev == dev, "the map is on %s, the frames on %s" % (mdev, dev)
    assert v.NMP >= 1, "empty map"
    lists = {k: t for k, t in lm.items() if k not in ("last_mp", "kf_feat_mp")}
    KFcap, NPcap = _check_lists(lists, B, v.NKF, dev)
    _tensor("lm['last_mp']", lm.get("last_mp"), "int32", (B, NL), dev)
    if fbk:
        _tensor("lm['kf_feat_mp']", lm.get("kf_feat_mp"), "int32", (B, NK), dev)
    out = _chain_out(a, NP=NPcap)
    out["feat_mp"] = torch.full((B, NF), -1, dtype=torch.int32, device=dev)
    io = _ChainIO()
    for k in CHAIN_FIELDS + CHAIN_FIELDS2A + CHAIN_FIELDS2B:
        if k in CHAIN_MAP_IGNORED:
            continue
        t = out["pose"] if k == "pose_cw" else (out[k] if k in out else a.get(k))
        setattr(io, k, _ptr(t) if t is not None else None)
    if fbk:
        io.NK, io.NNK, io.NNF = NK, a["kf_node_id"].shape[1], a["feat_node_id"].shape[1]
    l = _lib.gl_local_map_io()
    l.last_mp, l.kf_feat_mp, l.feat_mp, l.KFcap = _ptr(lm["last_mp"]), _ptr(lm["kf_feat_mp"]) if fbk else None, _ptr(out["feat_mp"]), KFcap
    for k in ("local_kf", "n_local_kf", "local_mp", "n_local_mp", "ref_kf", "kf_count", "status"):
        setattr(l, k, _ptr(lists[k]) if lists.get(k) is not None else None)
    ctx.call(ctx.lib.gl_track_frame_chain_map, C.byref(cam.c()), C.byref(prm.c()), float(scale_factor), B, NF, NL, NPcap, C.byref(io), C.byref(v),
             C.byref(l), float(th_mm), float(th_local), float(nn_ratio), int(bool(mono)))
    return out


# ---- the mapping thread on the resident map: covisibility, the local-BA window, the write-back (gmmloc_hip.h)
CONN_KEPT, CONN_TRUNCATED, CONN_BAD_ROW = 1, 2, 4
BA_WINDOW_NO_CONN, BA_WINDOW_P_TRUNCATED, BA_WINDOW_F_TRUNCATED, BA_WINDOW_L_TRUNCATED, BA_WINDOW_O_TRUNCATED, BA_WINDOW_BAD_ROW = 1, 2, 4, 8, 16, 32
BA_WINDOW_TRUNCATED, BA_WINDOW_DROPPED_SHIFT = 30, 8
BA_WINDOW_DTYPES = {"poses": "float64", "prior": "uint8", "points": "float64", "assoc": "int32", "obs_ptr": "int32", "obs_pose": "int32",
                    "obs_uvr": "float64", "obs_oct": "int32", "win_kf": "int32", "win_mp": "int32", "win_obs": "int32", "sizes": "int32",
                    "status": "int32"}


def update_connections(ctx, map, kf_row, Ccap=None, out=None, want_count=False):
    """gl_update_connections: KeyFrame::updateConnections (keyframe.cpp:243-316) for the B key-frame rows kf_row (B,) i32 on the map
    of update_local_map (rules and the tie rule - lowest row first: gmmloc_hip.h).  -> dict(conn_kf (B,Ccap), conn_w (B,Ccap), n_conn
    (B,) the true lengths, status (B,)[, kf_count (B,NKF)]); `out`: the same dict to write into (a key-frame with an empty counter
    keeps its lists)."""
    v, dev = _map_view(map, False)
    _tensor("kf_row", kf_row, "int32", (None,), dev)
    B = kf_row.shape[0]
    if out is not None:  # (its own capacity, and kf_count if it holds one)
        Ccap = _tensor("out['conn_kf']", out.get("conn_kf"), "int32", (B, None), dev).shape[1]
        want_count = out.get("kf_count") is not None
    assert Ccap is not None, "Ccap or out"
    spec = dict(conn_kf=("int32", (B, Ccap), -1), conn_w=("int32", (B, Ccap), 0), n_conn=("int32", (B,), 0), status=("int32", (B,), 0))
    if want_count:
        spec["kf_count"] = ("int32", (B, v.NKF), 0)
    out = _outputs(out, spec, dev)
    ctx.call(ctx.lib.gl_update_connections, C.byref(v), B, _ptr(kf_row), Ccap, _ptr(out["conn_kf"]), _ptr(out["conn_w"]), _ptr(out["n_conn"]),
             _ptr(out.get("kf_count")), _ptr(out["status"]))
    return out


def ba_window_slab(B, Pcap, Fcap, Lcap, Ocap, device="cuda"):
    """B empty local-BA slabs of these capacities (gl_ba_window: the arrays gl_joint_optimization takes, the back-maps win_kf / win_mp /
    win_obs, sizes, status) + the BA's outputs of the same capacities (dropped (B,Lcap) u8, erase (B,Ocap) u8, iters (B,)) and the
    write-back's (erase_obs (B,Ocap), n_erase (B,))."""
    import torch
    shapes = {"poses": (B, Pcap + Fcap, 7), "prior": (B, Pcap), "points": (B, Lcap, 3), "assoc": (B, Lcap), "obs_ptr": (B, Lcap + 1),
              "obs_pose": (B, Ocap), "obs_uvr": (B, Ocap, 3), "obs_oct": (B, Ocap), "win_kf": (B, Pcap + Fcap), "win_mp": (B, Lcap),
              "win_obs": (B, Ocap), "sizes": (B, 4), "status": (B,)}
    s = {k: torch.zeros(sh, dtype=getattr(torch, BA_WINDOW_DTYPES[k]), device=device) for k, sh in shapes.items()}
    s.update(dropped=torch.zeros((B, Lcap), dtype=torch.uint8, device=device), erase=torch.zeros((B, Ocap), dtype=torch.uint8, device=device),
             iters=torch.zeros(B, dtype=torch.int32, device=device), erase_obs=torch.zeros((B, Ocap), dtype=torch.int32, device=device),
             n_erase=torch.zeros(B, dtype=torch.int32, device=device))
    return s


def _ba_window(slab, dev):
    B, Pcap = _tensor("slab['prior']", slab.get("prior"), "uint8", (None, None), dev).shape
    PF = _tensor("slab['poses']", slab.get("poses"), "float64", (B, None, 7), dev).shape[1]
    Lcap = _tensor("slab['assoc']", slab.get("assoc"), "int32", (B, None), dev).shape[1]
    Ocap = _tensor("slab['obs_pose']", slab.get("obs_pose"), "int32", (B, None), dev).shape[1]
    assert PF >= Pcap, "slab['poses']: fewer poses than slab['prior'] has free ones"
    shapes = {"points": (B, Lcap, 3), "obs_ptr": (B, Lcap + 1), "obs_uvr": (B, Ocap, 3), "obs_oct": (B, Ocap), "win_kf": (B, PF), "win_mp": (B, Lcap),
              "win_obs": (B, Ocap), "sizes": (B, 4), "status": (B,)}
    w = _lib.gl_ba_window()
    w.Pcap, w.Fcap, w.Lcap, w.Ocap = Pcap, PF - Pcap, Lcap, Ocap
    for k, dt in BA_WINDOW_DTYPES.items():
        setattr(w, k, _ptr(_tensor("slab[%r]" % k, slab.get(k), dt, shapes[k], dev) if k in shapes else slab[k]))
    return w, B


def ba_window_build(ctx, map, ba, kf_row, slab):
    """gl_ba_window_build: the local-BA windows of the key-frame rows kf_row (B,) i32 from the resident map - the selection of
    Localization::jointOptimization (localization_opt.cpp:460-516) and its flattening (:639-763), reproduced quirks in gmmloc_hip.h.
    `map`: the dict of update_local_map + mp_pos; `ba`: dict(kf_pose (NKF,7), [kf_twc (NKF,3),] kf_uvr (NKF,NFK,3) f64, kf_oct (NKF,NFK),
    obs_feat (NOBS,), mp_assoc (NMP,) i32, kf_first int); `slab`: ba_window_slab's dict, written in place and returned (sizes (B,4) =
    the true P, F, L, nobs; status (B,))."""
    v, dev = _map_view(map, False)
    _tensor("map['mp_pos']", map.get("mp_pos"), "float64", (v.NMP, 3), dev)
    w = _map_ba_view(ba, v, dev)
    win, B = _ba_window(slab, dev)
    _tensor("kf_row", kf_row, "int32", (B,), dev)
    ctx.call(ctx.lib.gl_ba_window_build, C.byref(v), C.byref(w), B, _ptr(kf_row), C.byref(win))
    return slab


def ba_window_apply(ctx, map, ba, slab):
    """gl_ba_window_apply: the write-back of jointOptimization (:837-853, :898-922) from the slabs after the BA (slab['dropped'],
    ['erase'], ['iters'] = its outputs) onto the resident rows: ba['kf_pose'], ba['kf_twc'] (when given), map['mp_pos'], ba['mp_assoc'].
    -> (erase_obs (B,Ocap) i32: the CSR positions of the observations to remove, ascending; n_erase (B,)) = slab['erase_obs'], ['n_erase']."""
    v, dev = _map_view(map, False)
    _tensor("map['mp_pos']", map.get("mp_pos"), "float64", (v.NMP, 3), dev)
    w = _map_ba_view(ba, v, dev)
    win, B = _ba_window(slab, dev)
    _tensor("slab['dropped']", slab.get("dropped"), "uint8", (B, win.Lcap), dev)
    _tensor("slab['erase']", slab.get("erase"), "uint8", (B, win.Ocap), dev)
    _tensor("slab['iters']", slab.get("iters"), "int32", (B,), dev)
    _tensor("slab['erase_obs']", slab.get("erase_obs"), "int32", (B, win.Ocap), dev)
    _tensor("slab['n_erase']", slab.get("n_erase"), "int32", (B,), dev)
    ctx.call(ctx.lib.gl_ba_window_apply, C.byref(v), _ptr(map["mp_pos"]), C.byref(w), B, C.byref(win), _ptr(slab["dropped"]), _ptr(slab["erase"]),
             _ptr(slab["iters"]), _ptr(slab["erase_obs"]), _ptr(slab["n_erase"]))
    return slab["erase_obs"], slab["n_erase"]


def joint_optimization_from_map(ctx, gmm, cam, prm, map, ba, kf_row, caps, stop_flag=None, slab=None):
    """The local BA of ONE key-frame (row kf_row, an int) on the resident map, nothing flattened or uploaded by the host:
    ba_window_build -> the 16 bytes of `sizes` to the host -> gl_joint_optimization[_stoppable](B = 1) on the slab -> ba_window_apply.
    caps = (Pcap, Fcap, Lcap, Ocap); a window that exceeds one is built again, once, in a slab grown to its true sizes.  `slab`: a dict
    of ba_window_slab(1, ...) to reuse (a mapping thread keeps one).  -> dict(slab, P, F, L, nobs, status, caps (the capacities used);
    win_kf (P+F,), win_mp (L,), assoc_dropped (L,), obs_erase (nobs,), iters (1,), erase_obs (n_erase,) - views of the slab, for the
    host's own bookkeeping: removeObservation on erase_obs, before the next build)."""
    import torch
    v, dev = _map_view(map, False)
    _tensor("map['mp_pos']", map.get("mp_pos"), "float64", (v.NMP, 3), dev)
    w = _map_ba_view(ba, v, dev)
    caps = tuple(int(c) for c in caps)
    if slab is None:
        slab = ba_window_slab(1, *caps, device=dev)
    for attempt in range(2):
        win, B = _ba_window(slab, dev)
        assert B == 1, "slab: one window"
        if "kf_row" not in slab:
            slab["kf_row"] = torch.zeros(1, dtype=torch.int32, device=dev)
        slab["kf_row"].fill_(int(kf_row))
        ctx.call(ctx.lib.gl_ba_window_build, C.byref(v), C.byref(w), 1, _ptr(slab["kf_row"]), C.byref(win))
        # the one round trip: sizes and status to the host, a synchronise
        P, F, L, nobs, status = torch.cat((slab["sizes"][0], slab["status"])).tolist()
        if not status & BA_WINDOW_TRUNCATED:
            break
        assert attempt == 0, "the window still exceeds the capacities it asked for"
        caps = (max(caps[0], P), max(caps[1], F), max(caps[2], L), max(caps[3], nobs))
        slab = ba_window_slab(1, *caps, device=dev)
    assert not status & BA_WINDOW_BAD_ROW, "kf_row %d is not a key-frame row" % int(kf_row)
    s = slab
    for k in ("iters", "dropped", "erase"):  # (a reused slab: the BA's outputs start from zeros, as in joint_optimization)
        s[k].zero_()
    if L > 0 and nobs > 0:
        args = [gmm.h, C.byref(cam.c()), C.byref(prm.c()), 1, P, F, L, nobs, _ptr(s["poses"]), _ptr(s["prior"]), _ptr(s["points"]),
                _ptr(s["assoc"]), _ptr(s["obs_ptr"]), _ptr(s["obs_pose"]), _ptr(s["obs_uvr"]), _ptr(s["obs_oct"]), _ptr(s["dropped"]),
                _ptr(s["erase"]), _ptr(s["iters"])]
        if stop_flag is None:
            ctx.call(ctx.lib.gl_joint_optimization, *args)
        else:
            ctx.call(ctx.lib.gl_joint_optimization_stoppable, *args, _ptr(stop_flag))
    for k, sh in (("erase_obs", (1, win.Ocap)), ("n_erase", (1,))):
        _tensor("slab[%r]" % k, s.get(k), "int32", sh, dev)
    ctx.call(ctx.lib.gl_ba_window_apply, C.byref(v), _ptr(map["mp_pos"]), C.byref(w), 1, C.byref(win), _ptr(s["dropped"]), _ptr(s["erase"]),
             _ptr(s["iters"]), _ptr(s["erase_obs"]), _ptr(s["n_erase"]))
    n_erase = int(slab["n_erase"][0])
    return dict(slab=slab, P=P, F=F, L=L, nobs=nobs, status=status, caps=caps, win_kf=s["win_kf"][0, :P + F], win_mp=s["win_mp"][0, :L],
                assoc_dropped=s["dropped"][0, :L], obs_erase=s["erase"][0, :nobs], iters=s["iters"], erase_obs=s["erase_obs"][0, :n_erase])


# ---- editing the resident map: key-frame culling and removals (gmmloc_hip.h)
CULL_JUDGED, CULL_FIRST, CULL_BAD_ROW, CULL_INVALID, CULL_DUPLICATE = 0, 1, 2, 3, 4
CULL_MAX_KF = 524288
MAP_REMOVE_FIRST_REFUSED, MAP_REMOVE_DEAD_TRUNCATED = 1, 2
CULL_DTYPES = {"cull": "uint8", "num_mps": "int32", "num_redundant": "int32", "cand_status": "int32", "cull_rows": "int32"}


def cull_keyframes(ctx, map, ba, kf_depth, th_depth, cand, n_cand, out=None):
    """gl_cull_keyframes: Localization::removeKeyFrames (localization.cpp:334-399) for the B candidate lists cand (B,Ccap) i32 / n_cand
    (B,) i32 - conn_kf / n_conn of update_connections as they are - on the unedited map: the verdicts of the sequential loop in list
    order (rules, the weighted count, malformed input, the bound on NKF: gmmloc_hip.h).  kf_depth (NKF,NFK) f32; th_depth float.  The map
    is not modified.  -> dict(cull (B,Ccap) u8, num_mps, num_redundant, cand_status (B,Ccap) i32, cull_rows (B,Ccap) i32 + n_cull (B,):
    the culled rows in list order, what map_remove takes as rm_kf); `out`: the same dict to write into."""
    v, dev = _map_view(map, False)
    w = _map_ba_view(ba, v, dev, need=("kf_uvr", "kf_oct", "obs_feat"))
    _tensor("kf_depth", kf_depth, "float32", (v.NKF, v.NFK), dev)
    B, Ccap = _tensor("cand", cand, "int32", (None, None), dev).shape
    _tensor("n_cand", n_cand, "int32", (B,), dev)
    spec = {k: (dt, (B, Ccap), -1 if k == "cull_rows" else 0) for k, dt in CULL_DTYPES.items()}
    out = _outputs(out, dict(spec, n_cull=("int32", (B,), 0)), dev)
    ctx.call(ctx.lib.gl_cull_keyframes, C.byref(v), C.byref(w), _ptr(kf_depth), float(th_depth), B, max(Ccap, 1), _ptr(cand), _ptr(n_cand),
             _ptr(out["cull"]), _ptr(out["num_mps"]), _ptr(out["num_redundant"]), _ptr(out["cand_status"]), _ptr(out["cull_rows"]),
             _ptr(out["n_cull"]))
    return out


def _row_list(name, rows, n, dev):
    """a list of map_remove -> (pointer, count pointer, capacity)"""
    if rows is None:
        assert n is None, "n_%s without %s" % (name, name)
        return None, None, 0
    _tensor(name, rows, "int32", (None,), dev)
    return _ptr(rows), _count("n_" + name, n, dev), rows.shape[0]


def map_remove(ctx, map, ba, erase_obs=None, rm_kf=None, rm_mp=None, n_erase=None, n_rm_kf=None, n_rm_mp=None, mp_ref_kf=None, dead_cap=None,
               want_new_pos=False):
    """gl_map_remove: removals applied IN PLACE to the resident map - map['mp_valid'], ['kf_valid'] (both required here), ['kf_mp'],
    ['obs_ptr'], ['obs_kf'], ba['obs_feat'] and mp_ref_kf (NMP,) i32 when given: "the points of rm_mp, then the observations at the CSR
    positions erase_obs, then the key-frames rm_kf in list order" with the reference's cascade (a point left with a weighted count <= 2
    dies), the CSR compacted (rules: gmmloc_hip.h).  Each list: a 1-D i32 CUDA tensor, its length the tensor's or the device count n_x
    (a 1-element i32 tensor: n_erase of ba_window_apply, n_cull of cull_keyframes - no synchronise between the calls).
    -> dict(map, ba: the dicts with obs_kf / obs_feat cut to the new NOBS (views; everything else the same tensors), nobs, status,
    dead_mp (n_dead,) i32 ascending[, obs_new_pos (old NOBS,) i32]).  One 12-byte copy and one synchronise."""
    import torch
    v, dev = _map_view(map, False)
    _map_ba_view(ba, v, dev, need=("kf_uvr", "obs_feat"))
    assert map.get("mp_valid") is not None and map.get("kf_valid") is not None, "map_remove: mp_valid and kf_valid are written, both are needed"
    ed = _map_edit(map, ba, mp_ref_kf, v.NMP, dev)
    ls = _lib.gl_map_remove_lists()
    ls.rm_mp, ls.n_rm_mp, ls.rm_mp_cap = _row_list("rm_mp", rm_mp, n_rm_mp, dev)
    ls.erase_obs, ls.n_erase, ls.erase_cap = _row_list("erase_obs", erase_obs, n_erase, dev)
    ls.rm_kf, ls.n_rm_kf, ls.rm_kf_cap = _row_list("rm_kf", rm_kf, n_rm_kf, dev)
    dead_cap = v.NMP if dead_cap is None else int(dead_cap)
    result = torch.zeros(3, dtype=torch.int32, device=dev)
    dead = torch.zeros(dead_cap, dtype=torch.int32, device=dev)
    new_pos = torch.zeros(v.NOBS, dtype=torch.int32, device=dev) if want_new_pos else None
    o = _lib.gl_map_remove_out()
    o.result, o.dead_mp, o.obs_new_pos, o.dead_cap = _ptr(result), (_ptr(dead) if dead_cap else None), _ptr(new_pos), dead_cap
    ctx.call(ctx.lib.gl_map_remove, v.NMP, v.NKF, v.NFK, v.NOBS, C.byref(ed), _ptr(ba["kf_uvr"]), int(ba.get("kf_first", -1)), C.byref(ls),
             C.byref(o))
    nobs, n_dead, status = result.tolist()  # the one round trip
    r = dict(map=dict(map, obs_kf=map["obs_kf"][:nobs]), ba=dict(ba, obs_feat=ba["obs_feat"][:nobs]), nobs=nobs, status=status,
             dead_mp=dead[:min(n_dead, dead_cap)], n_dead=n_dead)
    if want_new_pos:
        r["obs_new_pos"] = new_pos
    return r


def mapping_pass_from_map(ctx, gmm, cam, prm, map, ba, kf_row, caps, kf_depth, th_depth, Ccap=64, mp_ref_kf=None, stop_flag=None, slab=None,
                          kf_tables=None, cov=None):
    """What Localization::spinOnce (localization.cpp:97-107) does to the map after a key-frame's local BA, on the resident map with nothing
    flattened or uploaded: joint_optimization_from_map -> map_remove(erase_obs) -> update_connections(kf_row) -> cull_keyframes on that
    list -> map_remove(rm_kf).  With kf_tables (dict(desc), as covis.refresh_points takes it) and mp_ref_kf, the window's points get their
    updateNormalAndDepth (localization_opt.cpp:921) behind the erase, as the reference has it; with cov (the graph of covis.py) the culled
    key-frames leave the stored graph too (covis.covis_remove, the graph part of Map::removeKeyFrame, map.cpp:77-87).  A host that keeps
    per-point normals or the graph on the device passes both; without them the two steps are the caller's.
    -> dict(ba: the dict of joint_optimization_from_map; map, ba_rows: the edited dicts; conn, cull: the dicts of update_connections /
    cull_keyframes (B = 1); the host's bookkeeping lists as int lists: erased (CSR positions of the map on entry), dead_by_erase, culled
    (key-frame rows in list order), dead_by_cull (map-point rows); status of the two removals[; covis_result: covis_remove's (4,) i32])."""
    import torch
    r = joint_optimization_from_map(ctx, gmm, cam, prm, map, ba, kf_row, caps, stop_flag=stop_flag, slab=slab)
    e = map_remove(ctx, map, ba, erase_obs=r["slab"]["erase_obs"][0], n_erase=r["slab"]["n_erase"], mp_ref_kf=mp_ref_kf)
    dev = map["obs_ptr"].device
    NMP, NKF = map["obs_ptr"].shape[0] - 1, map["kf_mp"].shape[0]
    if kf_tables is not None and mp_ref_kf is not None:
        from .covis import refresh_points
        refresh_points(ctx, e["map"], e["ba"], kf_tables, mp_ref_kf, (NMP, NKF, e["nobs"]), r["win_mp"], 2)
    conn = update_connections(ctx, e["map"], torch.full((1,), int(kf_row), dtype=torch.int32, device=dev), Ccap=Ccap)
    cull = cull_keyframes(ctx, e["map"], e["ba"], kf_depth, th_depth, conn["conn_kf"], conn["n_conn"])
    k = map_remove(ctx, e["map"], e["ba"], rm_kf=cull["cull_rows"][0], n_rm_kf=cull["n_cull"], mp_ref_kf=mp_ref_kf)
    out = {}
    if cov is not None:
        from .covis import covis_remove
        out["covis_result"] = covis_remove(ctx, cov, NKF, cull["cull_rows"][0], cull["n_cull"], int(ba.get("kf_first", -1)))
    n_cull = int(cull["n_cull"][0])
    return dict(ba=r, map=k["map"], ba_rows=k["ba"], conn=conn, cull=cull, erased=r["erase_obs"].tolist(), dead_by_erase=e["dead_mp"].tolist(),
                culled=cull["cull_rows"][0, :n_cull].tolist(), dead_by_cull=k["dead_mp"].tolist(), status=(e["status"], k["status"]), **out)


def search_by_projection_frame(ctx, cam, pose_cw, pose_lw, feat_uv, feat_ur, feat_oct, feat_angle, feat_desc, feat_taken,
                               last_pt, last_valid, last_oct, last_angle, last_desc, th=7.0, mono=False,
                               check_orientation=True, scale_factor=1.2):
    """ORBmatcher::searchByProjection(CurrentFrame, LastFrame, th, bMono) (orb_matcher.cpp:410-542) for B frame
    pairs -> (feat_match int32 (B,NF): index of the last-frame feature, nmatches int32 (B,))."""
    import torch
    B, NF = feat_oct.shape
    NL = last_oct.shape[1]
    match = torch.empty((B, NF), dtype=torch.int32, device=feat_oct.device)
    nm = torch.empty(B, dtype=torch.int32, device=feat_oct.device)
    ctx.call(ctx.lib.gl_search_by_projection_frame, C.byref(cam.c()), float(scale_factor), B, NF, NL, _ptr(pose_cw), _ptr(pose_lw), _ptr(feat_uv),
             _ptr(feat_ur), _ptr(feat_oct), _ptr(feat_angle), _ptr(feat_desc), _ptr(feat_taken), _ptr(last_pt), _ptr(last_valid), _ptr(last_oct),
             _ptr(last_angle), _ptr(last_desc), float(th), int(bool(mono)), int(bool(check_orientation)), _ptr(match), _ptr(nm))
    return match, nm


KF_KEYS = ("uv", "ur", "oct", "angle", "desc", "has_mp", "nnode", "node_id", "node_ptr", "node_idx")
KF_DTYPES = {"uv": "float64", "ur": "float32", "oct": "int32", "angle": "float32", "desc": "uint8", "has_mp": "uint8", "nnode": "int32",
             "node_id": "int32", "node_ptr": "int32", "node_idx": "int32"}


def _check_kf(kf, name, keys=KF_KEYS):
    """the key-frame tensors go to the library as raw pointers: a wrong dtype or a strided view would be read as garbage"""
    for k in keys:
        t, dt = kf[k], KF_DTYPES[k]
        assert t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch." + dt, "%s[%r]: expected a contiguous CUDA %s tensor, got %s" % (name, k, dt, t.dtype)


def search_for_triangulation(ctx, kf1, kf2, fmat, epipole, only_stereo=False, check_orientation=True, scale_factor=1.2):
    """ORBmatcher::searchForTriangulation (orb_matcher.cpp:141-293) for B key-frame pairs.  kf1 / kf2: dicts of CUDA tensors
    with the keys KF_KEYS - uv (B,N,2) f64, ur (B,N) f32, oct (B,N) i32, angle (B,N) f32, desc (B,N,32) u8, has_mp (B,N) u8 and
    the DBoW2 feature vector as CSR: nnode (B,) i32, node_id (B,NN) i32 ascending, node_ptr (B,NN+1) i32, node_idx (B,N) i32;
    fmat (B,9) f64, epipole (B,2) f32 -> (match12 int32 (B,N1): feature of key-frame 2 or -1, nmatches int32 (B,))."""
    import torch
    B, N1 = kf1["oct"].shape
    N2 = kf2["oct"].shape[1]
    NN1, NN2 = kf1["node_id"].shape[1], kf2["node_id"].shape[1]
    assert kf1["node_ptr"].shape[1] == NN1 + 1 and kf2["node_ptr"].shape[1] == NN2 + 1
    _check_kf(kf1, "kf1")
    _check_kf(kf2, "kf2")
    assert str(fmat.dtype) == "torch.float64" and str(epipole.dtype) == "torch.float32"
    dev = kf1["oct"].device
    match = torch.empty((B, N1), dtype=torch.int32, device=dev)
    nm = torch.empty(B, dtype=torch.int32, device=dev)
    ctx.call(ctx.lib.gl_search_for_triangulation, float(scale_factor), B, N1, N2, NN1, NN2, *[_ptr(kf1[k]) for k in KF_KEYS],
             *[_ptr(kf2[k]) for k in KF_KEYS], _ptr(fmat), _ptr(epipole), int(bool(only_stereo)), int(bool(check_orientation)), _ptr(match), _ptr(nm))
    return match, nm


def level_steps(scale_factor=1.2):
    """The seven steps of the predicted level (mappoint.cpp:289-293) with the host's logf: step[L] = largest ratio with level <= L."""
    out = np.zeros(7, np.float32)
    _check(_lib.load().gl_level_steps(float(scale_factor), out.ctypes.data_as(C.c_void_p)))
    return out


def project_map_points(ctx, cam, pose_cw, t_wc, pos, normal, max_dist, min_dist, cand, scale_factor=1.2):
    """Frame::project3 + MapPoint::checkScaleAndVisible for B frames x NP map points (tracking.cpp:233-256): CUDA tensors pose_cw (B,7),
    t_wc (B,3), pos / normal (B,NP,3) f64, max_dist / min_dist (B,NP) f32, cand (B,NP) u8 -> (uvr (B,NP,3), level int32 (B,NP),
    viewcos (B,NP), dist (B,NP), inview u8 (B,NP)): the mp_* inputs of search_by_projection / fuse_search."""
    import torch
    B, NP = cand.shape
    dev = cand.device
    uvr = torch.empty((B, NP, 3), dtype=torch.float64, device=dev)
    level = torch.empty((B, NP), dtype=torch.int32, device=dev)
    viewcos = torch.empty((B, NP), dtype=torch.float64, device=dev)
    dist = torch.empty((B, NP), dtype=torch.float64, device=dev)
    inview = torch.empty((B, NP), dtype=torch.uint8, device=dev)
    ctx.call(ctx.lib.gl_project_map_points, C.byref(cam.c()), float(scale_factor), B, NP, _ptr(pose_cw), _ptr(t_wc), _ptr(pos), _ptr(normal),
             _ptr(max_dist), _ptr(min_dist), _ptr(cand), _ptr(uvr), _ptr(level), _ptr(viewcos), _ptr(dist), _ptr(inview))
    return uvr, level, viewcos, dist, inview


MP_KF_DTYPES = {"twc": "float64", "valid": "uint8", "oct": "int32", "desc": "uint8"}
MP_DTYPES = {"pos": "float64", "valid": "uint8", "ref_kf": "int32", "obs_ptr": "int32", "obs_kf": "int32", "obs_feat": "int32"}
MP_OUT_DTYPES = {"desc": "uint8", "normal": "float64", "max_dist": "float32", "min_dist": "float32"}


def update_map_points(ctx, kf, mp, out, what=3, scale_factor=1.2):
    """MapPoint::computeDistinctiveDescriptors (mappoint.cpp:126-190, what & 1) and MapPoint::updateNormalAndDepth (:211-255, what & 2)
    for NP map points, in place (rules: gmmloc_hip.h, gl_update_map_points).  Dicts of CUDA tensors - kf: twc (NKF,3) f64, valid
    (NKF,) u8 (optional), oct (NKF,NFK) i32, desc (NKF,NFK,32) u8 (the feat_oct / feat_desc layout of fuse_search); mp: pos (NP,3)
    f64, valid (NP,) u8 (optional), ref_kf (NP,) i32, observations_ as CSR obs_ptr (NP+1,) i32, obs_kf / obs_feat (NOBS,) i32; out:
    desc (NP,32) u8, normal (NP,3) f64, max_dist / min_dist (NP,) f32 - the mp_* inputs of the matchers.  Keys `what` does not
    need may be left out."""
    for name, d, dtypes in (("kf", kf, MP_KF_DTYPES), ("mp", mp, MP_DTYPES), ("out", out, MP_OUT_DTYPES)):
        for k, t in d.items():
            if t is None:
                continue
            assert k in dtypes, "%s[%r]: unknown key" % (name, k)
            assert t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch." + dtypes[k], \
                "%s[%r]: expected a contiguous CUDA %s tensor, got %s" % (name, k, dtypes[k], t.dtype)
    ref = kf.get("desc") if kf.get("desc") is not None else kf.get("oct")
    NKF, NFK = (ref.shape[0], ref.shape[1]) if ref is not None else (kf["twc"].shape[0], 0)
    NP = mp["obs_ptr"].shape[0] - 1
    NOBS = mp["obs_kf"].shape[0] if mp.get("obs_kf") is not None else 0
    g = lambda d, k: _ptr(d.get(k))
    ctx.call(ctx.lib.gl_update_map_points, float(scale_factor), int(what), NP, NKF, NFK, NOBS, g(kf, "twc"), g(kf, "valid"), g(kf, "oct"),
             g(kf, "desc"), g(mp, "pos"), g(mp, "valid"), g(mp, "ref_kf"), g(mp, "obs_ptr"), g(mp, "obs_kf"), g(mp, "obs_feat"), g(out, "desc"),
             g(out, "normal"), g(out, "max_dist"), g(out, "min_dist"))
    return out


def fuse_search(ctx, cam, feat_uv, feat_ur, feat_oct, feat_desc, mp_uvr, mp_level, mp_valid, mp_desc, th=3.0, scale_factor=1.2):
    """Localization::fuseObservations (localization.cpp:226-318), the matching half, for B key-frames: CUDA tensors feat_uv (B,NF,2)
    f64, feat_ur (B,NF) f32, feat_oct (B,NF) i32, feat_desc (B,NF,32) u8; mp_uvr (B,NP,3) f64, mp_level (B,NP) i32, mp_valid (B,NP)
    u8, mp_desc (B,NP,32) u8 -> (best_idx int32 (B,NP) or -1, best_dist int32 (B,NP))."""
    import torch
    B, NF = feat_oct.shape
    NP = mp_level.shape[1]
    bi = torch.empty((B, NP), dtype=torch.int32, device=feat_oct.device)
    bd = torch.empty((B, NP), dtype=torch.int32, device=feat_oct.device)
    ctx.call(ctx.lib.gl_fuse_search, C.byref(cam.c()), float(scale_factor), B, NF, NP, _ptr(feat_uv), _ptr(feat_ur), _ptr(feat_oct), _ptr(feat_desc),
             _ptr(mp_uvr), _ptr(mp_level), _ptr(mp_valid), _ptr(mp_desc), float(th), _ptr(bi), _ptr(bd))
    return bi, bd


def search_by_bow(ctx, kf, fr, nn_ratio=0.7, check_orientation=True):
    """ORBmatcher::searchByBoW (orb_matcher.cpp:295-408) for B key-frame / frame pairs.  kf: dict of CUDA tensors angle (B,N1) f32,
    desc (B,N1,32) u8, has_mp (B,N1) u8 (valid map point) and the feature vector as CSR (nnode, node_id, node_ptr, node_idx, as in
    search_for_triangulation); fr: angle, desc and the feature vector of the frame -> (match21 int32 (B,N2): the key-frame feature
    whose map point the frame feature gets, or -1; nmatches int32 (B,))."""
    import torch
    B, N1 = kf["angle"].shape
    N2 = fr["angle"].shape[1]
    NN1, NN2 = kf["node_id"].shape[1], fr["node_id"].shape[1]
    assert kf["node_ptr"].shape[1] == NN1 + 1 and fr["node_ptr"].shape[1] == NN2 + 1
    _check_kf(kf, "kf", ("angle", "desc", "has_mp", "nnode", "node_id", "node_ptr", "node_idx"))
    _check_kf(fr, "fr", ("angle", "desc", "nnode", "node_id", "node_ptr", "node_idx"))
    dev = kf["angle"].device
    match = torch.empty((B, N2), dtype=torch.int32, device=dev)
    nm = torch.empty(B, dtype=torch.int32, device=dev)
    ctx.call(ctx.lib.gl_search_by_bow, float(nn_ratio), int(bool(check_orientation)), B, N1, N2, NN1, NN2,
             *[_ptr(kf[k]) for k in ("angle", "desc", "has_mp", "nnode", "node_id", "node_ptr", "node_idx")],
             *[_ptr(fr[k]) for k in ("angle", "desc", "nnode", "node_id", "node_ptr", "node_idx")], _ptr(match), _ptr(nm))
    return match, nm


def gather_triangulation_matches(ctx, match12, nmatches, side1, side2, cap=None):
    """gl_gather_triangulation_matches: the matches of search_for_triangulation as the per-match arrays of create_map_points.
    side1 / side2: dicts of CUDA tensors pose (B,7), uv (B,N,2), ur (B,N) f32, depth (B,N) f32, oct (B,N) i32, cand (B,N,k) i32,
    ncand (B,N) i32.  Returns (pair_off (B+1,), dict of the per-match tensors with `cap` rows)."""
    import torch
    B, N1 = match12.shape
    N2 = side2["oct"].shape[1]
    k = side1["cand"].shape[2]
    cap = cap if cap is not None else B * min(N1, N2)
    dev = match12.device
    off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    m = dict(pose1=torch.zeros((cap, 7), dtype=torch.float64, device=dev), uvr1=torch.zeros((cap, 3), dtype=torch.float64, device=dev),
             depth1=torch.zeros(cap, dtype=torch.float32, device=dev), oct1=torch.zeros(cap, dtype=torch.int32, device=dev),
             cand1=torch.zeros((cap, k), dtype=torch.int32, device=dev), n1=torch.zeros(cap, dtype=torch.int32, device=dev),
             pose2=torch.zeros((cap, 7), dtype=torch.float64, device=dev), uvr2=torch.zeros((cap, 3), dtype=torch.float64, device=dev),
             depth2=torch.zeros(cap, dtype=torch.float32, device=dev), oct2=torch.zeros(cap, dtype=torch.int32, device=dev),
             cand2=torch.zeros((cap, k), dtype=torch.int32, device=dev), n2=torch.zeros(cap, dtype=torch.int32, device=dev),
             pair=torch.full((cap,), -1, dtype=torch.int32, device=dev), idx1=torch.full((cap,), -1, dtype=torch.int32, device=dev),
             idx2=torch.full((cap,), -1, dtype=torch.int32, device=dev))
    keys = ("pose", "uv", "ur", "depth", "oct", "cand", "ncand")
    ctx.call(ctx.lib.gl_gather_triangulation_matches, B, N1, N2, k, cap, _ptr(match12), _ptr(nmatches), *[_ptr(side1[q]) for q in keys],
             *[_ptr(side2[q]) for q in keys], _ptr(off),
             *[_ptr(m[q]) for q in ("pose1", "uvr1", "depth1", "oct1", "cand1", "n1", "pose2", "uvr2", "depth2", "oct2", "cand2", "n2", "pair", "idx1", "idx2")])
    return off, m


def create_map_points(ctx, gmm, cam, prm, pose1, uvr1, depth1, oct1, pose2, uvr2, depth2, oct2, cand1, n1, cand2, n2,
                      scale_factor=1.2):
    """Localization::createMapPoints per-match block (localization_opt.cpp:286-420), N matches ->
    (x3d float64 (N,3), type int32 (N,), comp int32 (N,))."""
    import torch
    N, k = cand1.shape
    dev = pose1.device
    x3d = torch.empty((N, 3), dtype=torch.float64, device=dev)
    typ = torch.empty(N, dtype=torch.int32, device=dev)
    comp = torch.empty(N, dtype=torch.int32, device=dev)
    ctx.call(ctx.lib.gl_create_map_points, gmm.h, C.byref(cam.c()), C.byref(prm.c()), float(scale_factor), N, _ptr(pose1), _ptr(uvr1), _ptr(depth1),
             _ptr(oct1), _ptr(pose2), _ptr(uvr2), _ptr(depth2), _ptr(oct2), _ptr(cand1), _ptr(n1), _ptr(cand2), _ptr(n2), k, _ptr(x3d), _ptr(typ),
             _ptr(comp))
    return x3d, typ, comp



# the two depth-ordered walks (gl_create_stereo_points, gl_create_temporal_points) live in key_frame.py, as the calls that grow the map live
# in map_grow.py; they are part of this interface
from .key_frame import (STEREO_IN_DTYPES, STEREO_WALK_MAX, TEMPORAL_IN_DTYPES, TEMPORAL_LAST_DTYPES, create_stereo_points,  # noqa: E402, F401
                        create_temporal_points)
