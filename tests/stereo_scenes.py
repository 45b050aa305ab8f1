"""Random stereo scenes for gl_stereo_matches and the model (tests/stereo_ref.py): textured level images, the right one the left shifted by
an integer with noise, key-points with partner descriptors.  Test infrastructure; nothing in the product imports it.

A scene is a dict: cam (fx, bf, height), scale_factor, and `frame`: the keyword arguments of stereo_ref.stereo_matches."""
import numpy as np

from tests import stereo_ref

CAM = (100.0, 40.0)  # fx, bf: maxD = mbf / mb = 100 px
SHIFT = (12, 10, 8, 7, 6, 5, 4, 3)  # the right level image = the left one shifted by this many pixels (about 12 px at level 0)


def texture(rng, h, w):
    """independent random texture, lightly smoothed (a 3 x 3 box)"""
    t = rng.integers(0, 256, (h + 2, w + 2)).astype(np.int64)
    s = sum(t[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return ((2 * t[1:h + 1, 1:w + 1] + s // 9) // 3).astype(np.uint8)


def flip_bits(rng, desc, n):
    d = np.unpackbits(desc)
    d[rng.choice(256, n, replace=False)] ^= 1
    return np.packbits(d)


def random_scene(seed, size=(160, 120), nlevels=3, nfeat=120, scale_factor=1.2, displaced_every=9, orphan_every=13, nright=None, row=None):
    """nfeat left features on random levels, each with a partner on the right: same row, the level's shift to the left, a descriptor
    with 0 - 40 flipped bits.  Every `displaced_every`-th partner sits one pixel left of the feature instead - the true match is out
    of the slide's reach, so the correlation ends on an edge (:306), right of the feature (:325) or on a poor match for the median
    rule; every `orphan_every`-th has an unrelated descriptor (:261).  nright: the right side padded to that many key-points with
    unrelated ones.  row: every level-0 row coordinate is this one (all key-points in one band)."""
    rng = np.random.default_rng(seed)
    sf, _ = stereo_ref.scale_tables(scale_factor)
    W0, H0 = size
    left, right = [], []
    for l in range(nlevels):
        w, h = int(round(W0 / float(sf[l]))), int(round(H0 / float(sf[l])))
        img = texture(rng, h, w)
        shifted = np.empty_like(img)
        shifted[:, :w - SHIFT[l]] = img[:, SHIFT[l]:]
        shifted[:, w - SHIFT[l]:] = texture(rng, h, SHIFT[l])
        noisy = np.clip(shifted.astype(np.int64) + rng.integers(-6, 7, img.shape), 0, 255).astype(np.uint8)
        left.append(img)
        right.append(noisy)
    nright = nfeat if nright is None else nright
    feat_uv = np.zeros((nfeat, 2))
    feat_oct = np.zeros(nfeat, np.int32)
    feat_desc = rng.integers(0, 256, (nfeat, 32)).astype(np.uint8)
    r_uv = np.zeros((nright, 2), np.float32)
    r_oct = np.zeros(nright, np.int32)
    r_desc = rng.integers(0, 256, (nright, 32)).astype(np.uint8)
    for i in range(nfeat):
        l = int(rng.integers(0, nlevels))
        h, w = left[l].shape
        x, y = int(rng.integers(SHIFT[l] + 16, w - 16)), int(rng.integers(8, h - 8))
        if row is not None:
            y = int(round(row / float(sf[l])))
        s = float(sf[l])
        feat_uv[i] = ((x + rng.uniform(-0.3, 0.3)) * s, (y + rng.uniform(-0.3, 0.3)) * s)
        feat_oct[i] = l
        if i >= nright:
            continue
        xr = x - 1 if i % displaced_every == displaced_every - 1 else x - SHIFT[l]
        r_uv[i] = (np.float32((xr + rng.uniform(-0.3, 0.3)) * s), np.float32((y + rng.uniform(-0.6, 0.6)) * s))
        r_oct[i] = l
        if i % orphan_every != orphan_every - 1:
            r_desc[i] = flip_bits(rng, feat_desc[i], int(rng.integers(0, 41)))
    for i in range(nfeat, nright):
        l = int(rng.integers(0, nlevels))
        h, w = left[l].shape
        r_uv[i] = (np.float32(rng.uniform(0, w) * float(sf[l])), np.float32(rng.uniform(0, h) * float(sf[l])))
        r_oct[i] = l
    perm = rng.permutation(nright)  # the partner of feature i is NOT right key-point i
    frame = dict(feat_uv=feat_uv, feat_oct=feat_oct, feat_desc=feat_desc, r_uv=r_uv[perm], r_oct=r_oct[perm], r_desc=r_desc[perm],
                 pyr_left=left, pyr_right=right)
    return {"cam": CAM + (H0,), "scale_factor": scale_factor, "frame": frame}


_model = {}


def model_of(key, scene):
    """the model's outputs for a scene, computed once per process under `key` and read-only"""
    if key not in _model:
        out = stereo_ref.stereo_matches(scene["cam"], scene["scale_factor"], **scene["frame"])
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _model[key] = out
    return _model[key]
