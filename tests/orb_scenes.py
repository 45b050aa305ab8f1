"""Random scenes for gl_orb_describe and the model (tests/orb_ref.py): textured level images, key-points inside the 19-px margin with a few
outside it and on octaves that do not exist, a seeded synthetic pattern (the library ships none and the tests copy none).  The generator
keeps the condition of the issue: the double cos / sin of every described key-point's steering angle lie at least 2^-40 (relative) away
from a float rounding boundary, so that the device's and the host's libm cannot disagree; a key-point that fails it is moved.
Test infrastructure; nothing in the product imports it.

A scene is a dict: the keyword arguments of orb_ref.describe for ONE image."""
import numpy as np

from tests import orb_ref
from tests.stereo_scenes import texture


def synthetic_pattern(seed=31):
    """512 entries drawn uniformly from [-13, 13]^2"""
    return np.random.default_rng(seed).integers(-13, 14, (512, 2)).astype(np.int8)


PATTERN = synthetic_pattern()


def level_shapes(size, nlevels, scale_factor=1.2):
    sf = orb_ref.scale_table(scale_factor)
    return [(int(round(size[1] / float(sf[l]))), int(round(size[0] / float(sf[l])))) for l in range(nlevels)]


def random_scene(seed, size=(160, 120), nlevels=3, n=120, shapes=None, stray_every=11, empty_level=None, angles=False, blur_w=None, count=None):
    """n key-points on random levels (never on `empty_level`); every `stray_every`-th lies inside the margin or on an octave outside the
    pyramid.  shapes: the level shapes (h, w) instead of size / 1.2^l.  angles: kp_angle is given (random, with exact quarter turns).
    count: n_kp (the slots behind it hold key-points that WOULD be described)."""
    rng = np.random.default_rng(seed)
    shapes = level_shapes(size, nlevels) if shapes is None else shapes
    levels = [texture(rng, h, w) for h, w in shapes]
    choice = [l for l in range(len(shapes)) if l != empty_level and min(shapes[l]) >= 39]
    kp_xy, kp_oct = np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
    kp_angle = np.zeros(n, np.float32) if angles else None
    for i in range(n):
        while True:
            l = int(rng.choice(choice))
            h, w = shapes[l]
            x, y = int(rng.integers(19, w - 19)), int(rng.integers(19, h - 19))
            if angles:
                a = np.float32(rng.choice([0.0, 90.0, 180.0, 270.0]) if i % 7 == 0 else rng.uniform(0.0, 360.0))
            else:
                a = orb_ref.ic_angle(levels[l], x, y)[2]
            if orb_ref.trig_margin_ok(a):
                break
        if i % stray_every == stray_every - 1:
            kind = (i // stray_every) % 6
            if kind < 4:
                x, y = ((18, y), (w - 19, y), (x, 18), (x, h - 19))[kind]
            else:
                l = -1 if kind == 4 else len(shapes)
        kp_xy[i], kp_oct[i] = (x, y), l
        if angles:
            kp_angle[i] = a
    return dict(levels=levels, kp_xy=kp_xy, kp_oct=kp_oct, pattern=PATTERN, blur_w=orb_ref.default_blur(2.0) if blur_w is None else blur_w,
                scale_factor=1.2, n_kp=count, kp_angle=kp_angle)


_model = {}


def model_of(key, scene):
    """the model's outputs for a scene, computed once per process under `key` and read-only"""
    if key not in _model:
        out = orb_ref.describe(**scene)
        for v in out.values():
            v.setflags(write=False)
        _model[key] = out
    return _model[key]
