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


# ---- detection: gl_orb_pyramid, gl_orb_detect and the composite
DETECT_OUT = {"kp_xy": ("int32", 2, -1), "kp_oct": ("int32", None, -1), "kp_response": ("float32", None, 0.0)}  # per slot: dtype, trailing extent, padding


class RawPyramid:
    """what stereo.Pyramid is to uploaded levels, for a pyramid that is BUILT on the device: the buffer and its gl_image_pyramid"""

    def __init__(self, c, data, B):
        self.c, self.data, self.B = c, data, B
        self.shapes = [(c.height[l], c.width[l]) for l in range(c.nlevels)]


def pyramid_layout(width, height, nlevels=8, scale_factor=1.2, row_pad=0, lead=0):
    """gl_orb_pyramid_layout -> gl_image_pyramid without data: the level sizes of :1058-1060, levels one behind the other"""
    from .api import _check
    c = _lib.gl_image_pyramid()
    _check(_lib.load().gl_orb_pyramid_layout(int(width), int(height), int(nlevels), float(scale_factor), int(row_pad), int(lead), C.byref(c)))
    return c


def features_per_level(nfeatures, nlevels=8, scale_factor=1.2):
    """gl_orb_features_per_level: mnFeaturesPerLevel (:429-441)"""
    from .api import _check
    n = (C.c_int32 * 8)()
    _check(_lib.load().gl_orb_features_per_level(int(nfeatures), int(nlevels), float(scale_factor), n))
    return list(n)[:nlevels]


def detect_bound(pyr, nfeatures, scale_factor=1.2):
    """gl_orb_detect_bound: the most key-points each level can yield, max(N_l + 2, 4 nIni_l); their sum is the least N of detect"""
    from .api import _check
    n = (C.c_int32 * 8)()
    _check(_lib.load().gl_orb_detect_bound(C.byref(pyr.c), int(nfeatures), float(scale_factor), n))
    return list(n)[:pyr.c.nlevels]


def build_pyramid(ctx, images, nlevels=8, scale_factor=1.2, row_pad=0, lead=0, fill=0):
    """gl_orb_pyramid.  images (B,H,W) u8 CUDA tensor: the raw images.  -> RawPyramid: one device buffer, level 0 copied in (a device
    copy), levels 1 .. n - 1 resized on the device.  Nothing is read back."""
    import torch
    im = _tensor("images", images, "uint8", (None, None, None), None)
    B, H, W = im.shape
    c = pyramid_layout(W, H, nlevels, scale_factor, row_pad, lead)
    data = torch.full((B, c.frame_stride), fill, dtype=torch.uint8, device=im.device)
    data[:, c.offset[0]:c.offset[0] + H * c.stride[0]].view(B, H, c.stride[0])[:, :, :W] = im
    c.data = data.data_ptr()
    pyr = RawPyramid(c, data, B)
    ctx.call(ctx.lib.gl_orb_pyramid, B, C.byref(c), float(scale_factor))
    return pyr


def detect(ctx, pyr, nfeatures=1000, N=None, scale_factor=1.2, ini_th=20, min_th=7, cand_cap=8192, candidates=False, out=None):
    """gl_orb_detect on a pyramid of B images (RawPyramid or stereo.Pyramid).  N: the output capacity (None: the sum of detect_bound).
    -> dict(kp_xy (B,N,2) i32, kp_oct (B,N) i32, n_kp (B,) i32, kp_response (B,N) f32, level_count (B,8) i32, stat (B,4) i32) and, with
    candidates=True, cand_xy (B,8,cand_cap,2) i32, cand_resp (B,8,cand_cap) f32, cand_count (B,8) i32.  kp_xy / kp_oct / n_kp are
    describe's inputs as they stand.  Nothing is read back."""
    dev = pyr.data.device
    B = pyr.B
    if N is None:
        N = max(sum(detect_bound(pyr, nfeatures, scale_factor)), 1)
    spec = {k: (dt, (B, N) + ((tr,) if tr else ()), fill) for k, (dt, tr, fill) in DETECT_OUT.items()}
    spec.update(n_kp=("int32", (B,), 0), level_count=("int32", (B, 8), 0), stat=("int32", (B, 4), 0))
    if candidates:
        spec.update(cand_xy=("int32", (B, 8, cand_cap, 2), -1), cand_resp=("float32", (B, 8, cand_cap), 0.0), cand_count=("int32", (B, 8), 0))
    out = _outputs(out, spec, dev)
    o = _lib.gl_orb_detect_out()
    for key in spec:
        setattr(o, key, _ptr(out[key]))
    ctx.call(ctx.lib.gl_orb_detect, B, N, C.byref(pyr.c), int(nfeatures), float(scale_factor), int(ini_th), int(min_th), int(cand_cap), C.byref(o))
    return out


def extract(ctx, images, pattern, nfeatures=1000, nlevels=8, scale_factor=1.2, ini_th=20, min_th=7, cand_cap=8192, blur_w=None, N=None,
            out=None, detect_out=None):
    """ORBextractor::operator() for B raw images: gl_orb_pyramid -> gl_orb_detect -> gl_orb_describe on the context's stream; detect's
    kp_xy / kp_oct / n_kp are describe's inputs, the same device buffers, and no host read lies between the calls.  `out`: describe's
    (the chain's feat_desc / feat_angle / feat_uv under its keys).  -> (pyramid, detect's dict, describe's dict)"""
    pyr = build_pyramid(ctx, images, nlevels, scale_factor)
    det = detect(ctx, pyr, nfeatures, N, scale_factor, ini_th, min_th, cand_cap, out=detect_out)
    des = describe(ctx, det["kp_xy"], det["kp_oct"], pattern, pyr, blur_w=blur_w, scale_factor=scale_factor, n_kp=det["n_kp"], out=out)
    return pyr, det, des
