"""The two depth-ordered walks that make points from stereo depth, on the device: gl_create_stereo_points
(GMMLoc::createMapPointsFromStereo, gmmloc_opt.cpp:36-113) and gl_create_temporal_points (Tracking::createTemporalPoints,
tracking.cpp:411-465); rules in include/gmmloc_hip.h.  Reached as api.create_stereo_points / api.create_temporal_points; the composite
on the resident map is map_grow.process_key_frame_from_map.  Their pass over a context's history is
tests/test_gpu_key_frame_create_context.py."""
import ctypes as C

from . import _lib
from ._host import _outputs, _ptr, _tensor

STEREO_WALK_MAX = 4096  # GL_STEREO_WALK_MAX
STEREO_IN_DTYPES = {"pose": "float64", "feat_uv": "float64", "feat_ur": "float32", "feat_depth": "float32", "feat_oct": "int32", "cand": "int32",
                    "ncand": "int32", "held": "uint8", "kf_row": "int32"}
TEMPORAL_IN_DTYPES = {"pose": "float64", "feat_uv": "float64", "feat_depth": "float32", "feat_oct": "int32", "held": "uint8",
                      "last_outlier": "uint8", "feat_desc": "uint8"}
TEMPORAL_LAST_DTYPES = {"last_pt": "float64", "last_observed": "uint8", "last_valid": "uint8", "last_desc": "uint8"}


def _frame_shapes(B, NF, k=None):
    return {"pose": (B, 7), "feat_uv": (B, NF, 2), "feat_ur": (B, NF), "feat_depth": (B, NF), "feat_oct": (B, NF), "cand": (B, NF, k), "ncand": (B, NF),
            "held": (B, NF), "kf_row": (B,), "last_outlier": (B, NF), "feat_desc": (B, NF, 32), "last_pt": (B, NF, 3), "last_observed": (B, NF),
            "last_valid": (B, NF), "last_desc": (B, NF, 32)}


def create_stereo_points(ctx, gmm, cam, prm, kf, mp_base, check_depth, th_depth, want_pts0=False, out=None):
    """gl_create_stereo_points: GMMLoc::createMapPointsFromStereo (gmmloc_opt.cpp:36-113) for B key-frames (rules: gmmloc_hip.h).  kf:
    dict of CUDA tensors pose (B,7) f64, feat_uv (B,NF,2) f64, feat_ur / feat_depth (B,NF) f32, feat_oct (B,NF) i32, cand (B,NF,k) /
    ncand (B,NF) i32 (GMM.search2d), held (B,NF) u8 (0 null, 1 observed point, 2 point without observation), kf_row (B,) i32.
    -> dict of CUDA tensors: new_feat / new_assoc / new_ref_kf / att_mp / att_kf / att_feat (B,NF) i32 and new_pos (B,NF,3) f64, of
    which the first n_new[b] of row b are written (the rest is zero); n_new (B,) i32; feat_new (B,NF) i32; stats (B,8) i32[; pts0
    (B,NF,3) f64].  out: such a dict to write into instead of a fresh one.  Nothing is read back."""
    for key in kf:
        assert key in STEREO_IN_DTYPES, "kf[%r]: unknown key" % key
    dev = _tensor("kf['feat_oct']", kf.get("feat_oct"), "int32", (None, None), None).device
    B, NF = kf["feat_oct"].shape
    k = _tensor("kf['cand']", kf.get("cand"), "int32", (B, NF, None), dev).shape[2]
    shapes = _frame_shapes(B, NF, k)
    i = _lib.gl_stereo_points_in()
    for key, dt in STEREO_IN_DTYPES.items():
        setattr(i, key, _ptr(_tensor("kf[%r]" % key, kf.get(key), dt, shapes[key], dev)))
    spec = {key: ("int32", (B, NF), 0) for key in ("new_feat", "new_assoc", "new_ref_kf", "att_mp", "att_kf", "att_feat", "feat_new")}
    spec.update(new_pos=("float64", (B, NF, 3), 0), n_new=("int32", (B,), 0), stats=("int32", (B, 8), 0))
    if want_pts0 if out is None else out.get("pts0") is not None:
        spec["pts0"] = ("float64", (B, NF, 3), 0)
    r = _outputs(out, spec, dev)
    o = _lib.gl_stereo_points_out()
    for key in spec:
        setattr(o, key, _ptr(r[key]))
    ctx.call(ctx.lib.gl_create_stereo_points, gmm.h, C.byref(cam.c()), C.byref(prm.c()), B, NF, k, C.byref(i), int(mp_base), int(bool(check_depth)),
             float(th_depth), C.byref(o))
    return r


def create_temporal_points(ctx, cam, fr, last, th_depth, last_mp=None):
    """gl_create_temporal_points: Tracking::createTemporalPoints (tracking.cpp:411-465) for B last frames (rules: gmmloc_hip.h).  fr:
    dict of CUDA tensors pose (B,7) f64, feat_uv (B,NF,2) f64, feat_depth (B,NF) f32, feat_oct (B,NF) i32, held (B,NF) u8,
    last_outlier (B,NF) u8, feat_desc (B,NF,32) u8; last: the chain's last-frame arrays last_pt (B,NF,3) f64, last_observed /
    last_valid (B,NF) u8, last_desc (B,NF,32) u8, written IN PLACE for the created points.  -> dict(temp_flag (B,NF) u8, n_temp (B,)
    i32, stats (B,8) i32).  last_mp (B,NF) i32 or None: the slots' map rows (frame_step.frame_next's held_mp), set to -1 IN PLACE for the
    created points.  Nothing is read back."""
    import torch
    for key in fr:
        assert key in TEMPORAL_IN_DTYPES, "fr[%r]: unknown key" % key
    for key in last:
        assert key in TEMPORAL_LAST_DTYPES, "last[%r]: unknown key" % key
    dev = _tensor("fr['feat_oct']", fr.get("feat_oct"), "int32", (None, None), None).device
    B, NF = fr["feat_oct"].shape
    shapes = _frame_shapes(B, NF)
    i, o = _lib.gl_temporal_points_in(), _lib.gl_temporal_points_out()
    for key, dt in TEMPORAL_IN_DTYPES.items():
        setattr(i, key, _ptr(_tensor("fr[%r]" % key, fr.get(key), dt, shapes[key], dev)))
    for key, dt in TEMPORAL_LAST_DTYPES.items():
        setattr(o, key, _ptr(_tensor("last[%r]" % key, last.get(key), dt, shapes[key], dev)))
    r = dict(temp_flag=torch.zeros((B, NF), dtype=torch.uint8, device=dev), n_temp=torch.zeros(B, dtype=torch.int32, device=dev),
             stats=torch.zeros((B, 8), dtype=torch.int32, device=dev))
    for key, t in r.items():
        setattr(o, key, _ptr(t))
    if last_mp is not None:
        o.last_mp = _ptr(_tensor("last_mp", last_mp, "int32", (B, NF), dev))
    ctx.call(ctx.lib.gl_create_temporal_points, C.byref(cam.c()), B, NF, C.byref(i), float(th_depth), C.byref(o))
    return r
