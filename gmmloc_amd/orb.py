"""ORB orientation and descriptors on the device: gl_orb_describe, the regular half of ORBextractor (orb_extractor.cpp) for B images.
The rules and the declared deviations are in include/gmmloc_hip.h; this module enqueues the call on a stereo.Pyramid.  The library ships
no pattern: the host passes its own."""
import ctypes as C

from . import _lib
from ._host import _outputs, _ptr, _tensor

ORB_MAX = 4096  # GL_ORB_MAX


def default_blur(sigma=2.0):
    """gl_orb_default_blur: the Q8 taps of the 7-tap Gaussian, centre first (a declared rule; sigma = 2 -> [54, 49, 34, 18])"""
    from .api import _check
    w = (C.c_int32 * 4)()
    _check(_lib.load().gl_orb_default_blur(float(sigma), w))
    return list(w)


def describe(ctx, kp_xy, kp_oct, pattern, pyr, blur_w=None, scale_factor=1.2, n_kp=None, kp_angle=None, out=None):
    """gl_orb_describe.  kp_xy (B,N,2) i32: the key-points AT THEIR LEVEL in ROI coordinates, kp_oct (B,N) i32, pattern (512,2) i8, all
    CUDA tensors; pyr: stereo.Pyramid of B images; blur_w: four ints (None: default_blur(2)); n_kp (B,) i32 and kp_angle (B,N) f32 are
    optional.  -> dict(desc (B,N,32) u8, angle (B,N) f32, moments (B,N,2) i32, uv32 (B,N,2) f32, uv64 (B,N,2) f64, stat (B,2) i32);
    `out`: the dict of an earlier call (or the chain's feat_desc / feat_angle / feat_uv under these keys), written in place.  Nothing is
    read back except the pattern, once per context and pointer."""
    dev = _tensor("kp_oct", kp_oct, "int32", (None, None), None).device
    B, N = kp_oct.shape
    i, o = _lib.gl_orb_in(), _lib.gl_orb_out()
    i.kp_xy = _ptr(_tensor("kp_xy", kp_xy, "int32", (B, N, 2), dev))
    i.kp_oct = _ptr(kp_oct)
    i.pattern = _ptr(_tensor("pattern", pattern, "int8", (512, 2), dev))
    if n_kp is not None:
        i.n_kp = _ptr(_tensor("n_kp", n_kp, "int32", (B,), dev))
    if kp_angle is not None:
        i.kp_angle = _ptr(_tensor("kp_angle", kp_angle, "float32", (B, N), dev))
    w = (C.c_int32 * 4)(*(default_blur(2.0) if blur_w is None else [int(v) for v in blur_w]))
    i.blur_w = C.cast(w, C.POINTER(C.c_int32))
    i.scale_factor = float(scale_factor)
    assert pyr.B == B, "the pyramid holds %d images, the key-points %d" % (pyr.B, B)
    out = _outputs(out, {"desc": ("uint8", (B, N, 32), 0), "angle": ("float32", (B, N), -1.0), "moments": ("int32", (B, N, 2), 0),
                         "uv32": ("float32", (B, N, 2), -1.0), "uv64": ("float64", (B, N, 2), -1.0), "stat": ("int32", (B, 2), 0)}, dev)
    for key, _ in o._fields_:
        setattr(o, key, _ptr(out[key]))
    ctx.call(ctx.lib.gl_orb_describe, B, N, C.byref(i), C.byref(pyr.c), C.byref(o))
    return out
