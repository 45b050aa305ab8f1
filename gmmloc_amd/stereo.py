"""Stereo depth on the device: gl_stereo_matches, Frame::computeStereoMatches (frame.cpp:179-349) for B frames.  The rules and the
declared deviations are in include/gmmloc_hip.h; this module packs the image pyramids and enqueues the call."""
import ctypes as C

import numpy as np

from . import _lib
from ._host import _outputs, _ptr, _tensor

STEREO_MATCH_MAX = 4096  # GL_STEREO_MATCH_MAX
LEFT_DTYPES = {"feat_uv": "float64", "feat_oct": "int32", "feat_desc": "uint8"}
RIGHT_DTYPES = {"r_uv": "float32", "r_oct": "int32", "r_desc": "uint8"}


class Pyramid:
    """B frames' image pyramids in ONE device byte buffer with the struct that describes it (gl_image_pyramid).

    frames: a list (one entry per frame) of lists of level images, 2-D uint8 numpy arrays or tensors; every frame has the same level
    shapes.  row_pad: bytes added to every row (stride = width + row_pad), lead: bytes in front of level 0 - what a bordered buffer
    looks like.  The padding is filled with `fill`."""

    def __init__(self, frames, device, row_pad=0, lead=0, fill=0):
        import torch
        levels = [[np.asarray(im.cpu() if hasattr(im, "cpu") else im) for im in f] for f in frames]
        shapes = [im.shape for im in levels[0]]
        assert 1 <= len(shapes) <= 8, "a pyramid has 1 .. 8 levels"
        for f in levels:
            assert [im.shape for im in f] == shapes and all(im.dtype == np.uint8 and im.ndim == 2 for im in f), \
                "every frame: the same 2-D uint8 level images"
        c = _lib.gl_image_pyramid()
        c.nlevels = len(shapes)
        at = int(lead)
        for l, (h, w) in enumerate(shapes):
            c.width[l], c.height[l], c.stride[l], c.offset[l] = w, h, w + row_pad, at
            at += h * (w + row_pad)
        c.frame_stride = at
        buf = np.full((len(levels), at), fill, np.uint8)
        for b, f in enumerate(levels):
            for l, im in enumerate(f):
                rows = buf[b, c.offset[l]:c.offset[l] + im.shape[0] * c.stride[l]].reshape(im.shape[0], c.stride[l])
                rows[:, :im.shape[1]] = im
        self.data = torch.from_numpy(buf).to(device)
        c.data = self.data.data_ptr()
        self.c, self.B, self.shapes = c, len(levels), shapes


def stereo_matches(ctx, cam, left, right, pyr_left, pyr_right, scale_factor=1.2, out=None):
    """gl_stereo_matches.  left: dict of CUDA tensors feat_uv (B,NF,2) f64, feat_oct (B,NF) i32, feat_desc (B,NF,32) u8 - the chain's
    own buffers - and optionally n_left (B,) i32; right: r_uv (B,NR,2) f32, r_oct (B,NR) i32, r_desc (B,NR,32) u8, optionally n_right.
    pyr_left / pyr_right: Pyramid.  -> dict(feat_ur, feat_depth (B,NF) f32, match_r, sad (B,NF) i32, stat (B,4) i32); `out`: the dict
    of an earlier call (or the chain's feat_ur / the frame step's feat_depth under those keys), written in place.  Nothing is read back."""
    dev = _tensor("left['feat_oct']", left.get("feat_oct"), "int32", (None, None), None).device
    B, NF = left["feat_oct"].shape
    NR = _tensor("right['r_oct']", right.get("r_oct"), "int32", (B, None), dev).shape[1]
    shapes = {"feat_uv": (B, NF, 2), "feat_oct": (B, NF), "feat_desc": (B, NF, 32), "r_uv": (B, NR, 2), "r_oct": (B, NR), "r_desc": (B, NR, 32)}
    i, o = _lib.gl_stereo_in(), _lib.gl_stereo_out()
    for side, name, dtypes, count in ((left, "left", LEFT_DTYPES, "n_left"), (right, "right", RIGHT_DTYPES, "n_right")):
        for key in side:
            assert key in dtypes or key == count, "%s[%r]: unknown key" % (name, key)
        for key, dt in dtypes.items():
            setattr(i, key, _ptr(_tensor("%s[%r]" % (name, key), side.get(key), dt, shapes[key], dev)))
        if side.get(count) is not None:
            setattr(i, count, _ptr(_tensor("%s[%r]" % (name, count), side[count], "int32", (B,), dev)))
    assert pyr_left.B == B and pyr_right.B == B, "the pyramids hold %d / %d frames, the features %d" % (pyr_left.B, pyr_right.B, B)
    out = _outputs(out, {"feat_ur": ("float32", (B, NF), -1.0), "feat_depth": ("float32", (B, NF), -1.0), "match_r": ("int32", (B, NF), -1),
                         "sad": ("int32", (B, NF), -1), "stat": ("int32", (B, 4), 0)}, dev)
    for key, _ in o._fields_:
        setattr(o, key, _ptr(out[key]))
    ctx.call(ctx.lib.gl_stereo_matches, C.byref(cam.c()), float(scale_factor), B, NF, NR, C.byref(i), C.byref(pyr_left.c), C.byref(pyr_right.c),
             C.byref(o))
    return out
