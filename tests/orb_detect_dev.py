"""gl_orb_pyramid / gl_orb_detect on images of the model's form (tests/orb_detect_ref.py): upload, call, guard words, read back, and the
model's outputs in the call's layout - stated once for the GPU test modules of the two calls.  Test infrastructure; nothing in the
product imports it."""
import functools

import numpy as np

from tests import orb_detect_ref as ref
from tests.orb_dev import _GUARD, GUARD, guarded

SLOT = {"kp_xy": ("int32", 2, -1), "kp_oct": ("int32", None, -1), "kp_response": ("float32", None, 0.0)}
KEYS = ("kp_xy", "kp_oct", "n_kp", "kp_response", "level_count", "stat", "cand_xy", "cand_resp", "cand_count")


def scene(seed, size=(160, 120), grain=2, contrast=1.0):
    """a textured image: noise of `grain` px blocks under a little pixel noise, so that FAST finds corners at both thresholds"""
    rng = np.random.default_rng(seed)
    w, h = size
    coarse = rng.integers(0, 256, ((h + grain - 1) // grain, (w + grain - 1) // grain)).astype(np.float64)
    img = np.kron(coarse, np.ones((grain, grain)))[:h, :w]
    img = 128 + (img - 128) * contrast + rng.integers(-6, 7, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def model(key, nfeatures, cand_cap, ini_th=20, min_th=7):
    """the model's outputs for the image registered under `key` (IMAGES), computed once per process"""
    return ref.detect(IMAGES[key], nfeatures, 1.2, ini_th, min_th, cand_cap)


IMAGES = {}  # key -> the levels of one image


def register(key, levels):
    if key not in IMAGES:
        IMAGES[key] = [np.ascontiguousarray(l) for l in levels]
        for l in IMAGES[key]:
            l.setflags(write=False)
    return key


def expected(models, N, cand_cap):
    """the models' outputs stacked in the call's layout"""
    B = len(models)
    r = {"n_kp": np.array([len(m["kp_oct"]) for m in models], np.int32), "level_count": np.stack([m["level_count"] for m in models]),
         "stat": np.stack([m["stat"] for m in models]), "cand_count": np.stack([m["cand_count"] for m in models]),
         "cand_xy": np.full((B, 8, cand_cap, 2), -1, np.int32), "cand_resp": np.zeros((B, 8, cand_cap), np.float32)}
    for k, (dt, trail, fill) in SLOT.items():
        r[k] = np.full((B, N) + ((trail,) if trail else ()), fill, dt)
        for b, m in enumerate(models):
            r[k][b, :len(m[k])] = m[k]
    for b, m in enumerate(models):
        for l, c in enumerate(m["cand"]):
            n = min(len(c), cand_cap)
            r["cand_xy"][b, l, :n] = c[:n, :2]
            r["cand_resp"][b, l, :n] = c[:n, 2]
    return r


def run(torch, ctx, frames, nfeatures, N, cand_cap, ini_th=20, min_th=7, row_pad=0, lead=0):
    """frames: a list of level lists.  -> the call's outputs as numpy arrays; asserts that the guard words behind every output are
    intact and that the pyramid has not changed"""
    from gmmloc_amd import orb, stereo
    dev = torch.device("cuda:0")
    pyr = stereo.Pyramid(frames, dev, row_pad=row_pad, lead=lead, fill=0xAB)
    before = pyr.data.cpu().numpy().copy()
    B = len(frames)
    shapes = {"n_kp": ((B,), "int32"), "level_count": ((B, 8), "int32"), "stat": ((B, 4), "int32"), "cand_count": ((B, 8), "int32"),
              "cand_xy": ((B, 8, cand_cap, 2), "int32"), "cand_resp": ((B, 8, cand_cap), "float32")}
    shapes.update({k: ((B, N) + ((tr,) if tr else ()), dt) for k, (dt, tr, _) in SLOT.items()})
    out, whole = {}, {}
    for k, (sh, dt) in shapes.items():
        out[k], whole[k] = guarded(torch, sh, dt, dev)
    orb.detect(ctx, pyr, nfeatures, N, 1.2, ini_th, min_th, cand_cap, candidates=True, out=out)
    ctx.synchronize()
    got = {k: out[k].cpu().numpy() for k in KEYS}
    for k in KEYS:
        tail = whole[k][-GUARD:].cpu().numpy()
        assert np.all(tail == tail.dtype.type(_GUARD[str(tail.dtype)])), "guard words behind %s overwritten" % k
    assert np.array_equal(pyr.data.cpu().numpy(), before), "the pyramid changed"
    return got


def same_bits(got, want, label, keys=KEYS):
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (label, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)
            first = tuple(bad[0]) if len(bad) else ()
            raise AssertionError("%s, output %s: %d of %d elements differ, first at %s: device %r, expected %r" %
                                 (label, k, len(bad), a.size, first, a[first] if first else None, b[first] if first else None))


def run_pyramid(torch, ctx, images, nlevels, row_pad=0, lead=0, scale_factor=1.2):
    """gl_orb_pyramid on raw images (B x H x W uint8) -> the levels of every frame as numpy arrays; asserts that every byte outside
    levels 1 .. n - 1 keeps its value"""
    from gmmloc_amd import orb
    dev = torch.device("cuda:0")
    pyr = orb.build_pyramid(ctx, torch.from_numpy(np.stack(images)).to(dev), nlevels, scale_factor, row_pad, lead, fill=0xAB)
    ctx.synchronize()
    buf = pyr.data.cpu().numpy()
    c = pyr.c
    mask = np.ones(buf.shape[1], bool)
    frames = [[] for _ in images]
    for l in range(nlevels):
        h, w, st, off = c.height[l], c.width[l], c.stride[l], c.offset[l]
        for b in range(len(images)):
            frames[b].append(buf[b, off:off + h * st].reshape(h, st)[:, :w].copy())
        if l:
            mask[off:off + h * st].reshape(h, st)[:, :w] = False
    for b, im in enumerate(images):
        assert np.array_equal(frames[b][0], im), "level 0 changed"
        rest = buf[b][mask].copy()
        h, st, off = c.height[0], c.stride[0], c.offset[0]
        keep = np.ones(buf.shape[1], bool)
        keep[off:off + h * st].reshape(h, st)[:, :c.width[0]] = False
        assert np.all(buf[b][mask & keep] == 0xAB), "a byte outside the levels was written"
    return frames
