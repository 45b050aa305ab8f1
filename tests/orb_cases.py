"""Hand-built cases of gl_orb_describe, each with DECLARED outputs: the numbers below are worked out by hand from the rules in
include/gmmloc_hip.h, not taken from the model (tests/test_orb_ref.py holds the model to them, tests/test_gpu_orb.py the device to the
model).  Images are 39 x 39 (a key-point at (19, 19) is the only one its level admits) to 64 x 48.

A case: group (the call's pattern, blur weights and level shapes: cases of one group run as one batch), levels, kp_xy, kp_oct, kp_angle
(None: the orientation is computed) and expect: desc, moments, uv32, uv64, stat exactly; `angle` exactly where the declared fastAtan2
gives it without arithmetic (0 / 90 / 180 / 270, a skipped slot's -1, a passed kp_angle) and `angle_near` (degrees, atan2) elsewhere:
the declared polynomial stays within orb_ref.ANGLE_BOUND of it.  Test infrastructure; nothing in the product imports it."""
import math

import numpy as np

from tests import orb_ref

f32 = np.float32
UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]  # the header's table
SF = [1.0, 1.2000000476837158, 1.440000057220459, 1.7280000448226929, 2.0736000537872314, 2.4883201122283936, 2.9859840869903564,
      3.5831809043884277]  # the extractor's level table for 1.2, as floats
IDENTITY, SIGMA2 = [256, 0, 0, 0], [54, 49, 34, 18]  # (256 * 256 p + 2^15) >> 16 = p;  gl_orb_default_blur(2)
HALF_PLANE = 255 * 2448  # 255 x sum over the patch's rows of u_max (u_max + 1) / 2 = 255 x sum of v (2 u_max[v] + 1): both are 2 448
C = 19  # the key-point of a 39 x 39 level


def pattern_of(pairs):
    """512 x 2 int8, zero but for pair q (samples 2 q, 2 q + 1) = pairs[q]"""
    p = np.zeros((512, 2), np.int8)
    for q, (s0, s1) in pairs.items():
        p[2 * q], p[2 * q + 1] = s0, s1
    return p


def desc_of(byte0):
    d = np.zeros(32, np.uint8)
    d[0] = byte0
    return d


def image(h=39, w=39, fill=0, **pixels):
    """pixels: r<row>c<col>=value"""
    im = np.full((h, w), fill, np.uint8)
    for k, v in pixels.items():
        r, c = k[1:].split("c")
        im[int(r), int(c)] = v
    return im


def find_half_angle():
    """the float angle nearest 30 degrees whose steering sine is exactly 0.5f (the generator SEARCHES and asserts)"""
    for away in (np.inf, -np.inf):
        a = f32(30.0)
        for _ in range(64):
            if orb_ref.steer(a)[1] == f32(0.5) and orb_ref.trig_margin_ok(a):
                return a
            a = np.nextafter(a, f32(away))
    raise AssertionError("no float near 30 degrees steers with b == 0.5f")


HALF_ANGLE = find_half_angle()
# an angle and a pattern entry at which fmaf(x, a, -(y * b)) and x * a - y * b round to different columns (found by a search over the
# angles k / 10 000 and all entries; asserted in tests/test_orb_ref.py): entry (11, 5) is read at (row 6, column 10), contracted (6, 11)
CONTRACT_ANGLE, CONTRACT_ENTRY = f32(5.215), (11, 5)

GROUPS = {
    "orient": dict(pattern=pattern_of({}), blur_w=SIGMA2),
    "axis": dict(pattern=pattern_of({0: ((5, 0), (0, 0)), 1: ((0, 5), (0, 0)), 2: ((5, 0), (0, 5))}), blur_w=IDENTITY),
    "half": dict(pattern=pattern_of({0: ((1, 0), (3, 0))}), blur_w=IDENTITY),
    "equal": dict(pattern=pattern_of({0: ((2, 0), (0, 2)), 1: ((0, 2), (2, 0))}), blur_w=IDENTITY),
    "extreme": dict(pattern=pattern_of({0: ((13, 13), (-13, -13)), 1: ((13, -13), (-13, 13)), 2: ((-13, -13), (13, 13))}), blur_w=IDENTITY),
    "contract": dict(pattern=pattern_of({0: (CONTRACT_ENTRY, (0, 0))}), blur_w=IDENTITY),
    "edge": dict(pattern=pattern_of({0: ((0, 0), (5, 0))}), blur_w=IDENTITY),
    "octaves": dict(pattern=pattern_of({0: ((0, 0), (5, 0))}), blur_w=IDENTITY),
    "impulse": dict(pattern=pattern_of({0: ((0, 0), (-13, -13)), 1: ((1, 0), (0, 0)), 2: ((-13, -13), (0, 0))}), blur_w=SIGMA2),
    "sum256": dict(pattern=pattern_of({0: ((0, 0), (5, 0))}), blur_w=SIGMA2),
    "sum257": dict(pattern=pattern_of({0: ((0, 0), (5, 0))}), blur_w=[55, 49, 34, 18]),
    "rounding": dict(pattern=pattern_of({0: ((5, 0), (0, 0))}), blur_w=[16, 0, 0, 0]),
}
CASES = {}
BLURRED = {}  # case -> the DECLARED blurred level 0 (the blur cases)


def case(name, group, levels, kps, expect, angles=None):
    """kps: (x, y, octave) per key-point; expect: per key-point dicts (None: skipped), made into arrays here"""
    n = len(kps)
    e = dict(desc=np.zeros((n, 32), np.uint8), moments=np.zeros((n, 2), np.int32), uv32=np.full((n, 2), -1.0, f32), angle=np.full(n, np.nan, f32),
             angle_near=np.full(n, np.nan))
    for i, x in enumerate(expect):
        if x is None:
            e["angle"][i] = -1.0
            continue
        e["desc"][i] = desc_of(x.get("byte0", 0))
        e["moments"][i] = x.get("moments", (0, 0))
        e["uv32"][i] = x["uv"]
        if "angle" in x:
            e["angle"][i] = x["angle"]
        else:
            e["angle_near"][i] = x["angle_near"]
    e["uv64"] = e["uv32"].astype(np.float64)
    e["stat"] = np.array([sum(x is not None for x in expect), sum(x is None for x in expect)], np.int32)
    assert name not in CASES and all(39 <= im.shape[1] <= 64 and 39 <= im.shape[0] <= 48 for im in levels)
    CASES[name] = dict(group=group, levels=levels, kp_xy=np.array([k[:2] for k in kps], np.int32).reshape(n, 2),
                       kp_oct=np.array([k[2] for k in kps], np.int32), kp_angle=None if angles is None else np.array(angles, f32), expect=e)


def at_centre(**x):
    return dict(uv=(C, C), **x)


# ---- orientation: m_10 = sum u I, m_01 = sum v I over the rows |u| <= u_max[|v|]
for v in range(-15, 16):
    for s in (-1, 1):
        u = s * UMAX[abs(v)]
        # a single bright pixel at the end of patch row v: it alone counts
        case("row%+03d end%+d" % (v, s), "orient", [image(**{"r%dc%d" % (C + v, C + u): 255})], [(C, C, 0)],
             [at_centre(moments=(255 * u, 255 * v), angle_near=math.degrees(math.atan2(v, u)) % 360.0)])
        # and one pixel beyond it: nothing counts, fastAtan2(0, 0) = 0
        case("row%+03d beyond%+d" % (v, s), "orient", [image(**{"r%dc%d" % (C + v, C + u + s): 255})], [(C, C, 0)], [at_centre(angle=0.0)])
case("uniform", "orient", [image(fill=200)], [(C, C, 0)], [at_centre(angle=0.0)])  # every u and v cancels
for name, sel, mom, ang in (("right", np.s_[:, C + 1:], (HALF_PLANE, 0), 0.0), ("below", np.s_[C + 1:, :], (0, HALF_PLANE), 90.0),
                            ("left", np.s_[:, :C], (-HALF_PLANE, 0), 180.0), ("above", np.s_[:C, :], (0, -HALF_PLANE), 270.0)):
    im = image()
    im[sel] = 255
    case("half-plane " + name, "orient", [im], [(C, C, 0)], [at_centre(moments=mom, angle=ang)])  # the largest moment: 624 240 < 2^24

# ---- descriptor, steered through kp_angle (moments stay 0).  Identity blur: the samples are the image's own pixels.
# angle 0: (x, y) is read at row y, column x; 90: row x, column -y; 180: row -y, column -x; 270: row -x, column y
AXIS = image(r19c19=25, r19c24=10, r24c19=20, r19c14=30, r14c19=40)
case("axes", "axis", [AXIS], [(C, C, 0)] * 4,
     [at_centre(angle=0.0, byte0=0b111),      # (5,0) -> 10, (0,5) -> 20: 10 < 25, 20 < 25, 10 < 20
      at_centre(angle=90.0, byte0=0b101),     # (5,0) -> 20, (0,5) -> 30: 20 < 25, 30 < 25 fails, 20 < 30
      at_centre(angle=180.0, byte0=0b100),    # (5,0) -> 30, (0,5) -> 40: both fail against 25, 30 < 40
      at_centre(angle=270.0, byte0=0b010)],   # (5,0) -> 40, (0,5) -> 10: 40 < 25 fails, 10 < 25, 40 < 10 fails
     angles=[0.0, 90.0, 180.0, 270.0])
# b == 0.5f: entry (1, 0) is read at row cvRound(0.5) = 0 (half to even; half away from zero: 1), column cvRound(0.866) = 1; entry
# (3, 0) at row cvRound(1.5) = 2 (either way), column cvRound(2.598) = 3
case("half to even", "half", [image(r19c20=50, r20c20=200, r21c22=100)], [(C, C, 0)], [at_centre(angle=HALF_ANGLE, byte0=1)], angles=[HALF_ANGLE])
case("t0 == t1", "equal", [image(r19c21=77, r21c19=77)], [(C, C, 0)], [at_centre(angle=0.0, byte0=0)], angles=[0.0])
# 45 degrees: (13, 13) -> row cvRound(18.38) = 18, column 0; (-13, -13) -> row -18; (13, -13) -> column 18; (-13, 13) -> column -18
case("extremes", "extreme", [image(r37c19=10, r1c19=20, r19c37=30, r19c1=40)], [(C, C, 0)], [at_centre(angle=45.0, byte0=0b011)], angles=[45.0])
case("no contraction", "contract", [image(r19c19=100, r25c29=50, r25c30=200)], [(C, C, 0)], [at_centre(angle=CONTRACT_ANGLE, byte0=1)],
     angles=[CONTRACT_ANGLE])
# the border: I = the column index, bit 0 = I(x) < I(x + 5) = 1 for a key-point that is described
RAMP = np.tile(np.arange(64, dtype=np.uint8), (48, 1))
case("19 px and 18 px", "edge", [RAMP], [(19, 19, 0), (18, 19, 0), (44, 28, 0), (45, 28, 0), (19, 29, 0), (19, 18, 0)],
     [dict(uv=(19, 19), angle=0.0, byte0=1), None, dict(uv=(44, 28), angle=0.0, byte0=1), None, None, None], angles=[0.0] * 6)
case("every octave", "octaves", [RAMP[:39, :39] + np.uint8(l) for l in range(8)], [(C, C, l) for l in (0, 1, 2, 3, 4, 5, 6, 7, -1, 8)],
     [dict(uv=(f32(C) * f32(SF[l]),) * 2, angle=0.0, byte0=1) for l in range(8)] + [None, None], angles=[0.0] * 10)

# ---- the blur.  A 1-D impulse answers with the taps 18 34 49 54 49 34 18 around it; REFLECT_101 never reads the edge pixel twice, so
# at index 0 the answer is 54 49 34 18 (BORDER_REFLECT would give 103 ...).  2-D: (255 r_y r_x + 2^15) >> 16.
def impulse_response(py, px):
    def one(p):
        r = np.zeros(39, np.int64)
        for k, t in zip(range(-3, 4), (18, 34, 49, 54, 49, 34, 18)):
            if 0 <= p + k < 39:
                r[p + k] = t
        return r
    return np.minimum((255 * np.outer(one(py), one(px)) + (1 << 15)) >> 16, 255).astype(np.uint8)


# 45 degrees: pair 0 = centre against (-13, -13) -> (row 1, column 19); pair 1 = (1, 0) -> (row 20, column 20) against the centre; pair 2
# = pair 0 the other way round
for name, (py, px), byte0 in (("corner", (0, 0), 0b000),   # out of every sample's reach: 0 < 0 fails three times
                              ("edge", (0, 19), 0b001),    # (1, 19) holds (255 x 49 x 54 + 2^15) >> 16 = 10: 0 < 10
                              ("centre", (19, 19), 0b110)):  # centre 11, (20, 20) holds (255 x 49 x 49 + 2^15) >> 16 = 9: 9 < 11, 0 < 11
    case("impulse " + name, "impulse", [image(**{"r%dc%d" % (py, px): 255})], [(C, C, 0)], [at_centre(angle=45.0, byte0=byte0)], angles=[45.0])
    BLURRED["impulse " + name] = impulse_response(py, px)
# both impulses (their answers do not overlap): (1, 19) holds 10 and the centre 11, so 11 < 10 fails, 9 < 11, 10 < 11.  Under
# BORDER_REFLECT row 1 would answer the impulse in row 0 with 49 + 34 = 83 and (1, 19) would hold 17
case("impulse edge and centre", "impulse", [image(r0c19=255, r19c19=255)], [(C, C, 0)], [at_centre(angle=45.0, byte0=0b110)], angles=[45.0])
BLURRED["impulse edge and centre"] = impulse_response(0, 19) + impulse_response(19, 19)
# 255 everywhere: 255 x 256 x 256 = 255 << 16 exactly; 255 x 257 x 257 >> 16 = 257, saturated to 255: no bit is set either way
for g in ("sum256", "sum257"):
    case("uniform 255, " + g, g, [image(fill=255)], [(C, C, 0)], [at_centre(angle=0.0, byte0=0)], angles=[0.0])
    BLURRED["uniform 255, " + g] = np.full((39, 39), 255, np.uint8)
# 128 x 16 x 16 = 2^15: (2^15 + 2^15) >> 16 = 1 (a rounding constant of 2^15 - 1 gives 0), right of column 19 the image is 0
im = image()
im[:, :C + 1] = 128
case("rounding constant", "rounding", [im], [(C, C, 0)], [at_centre(angle=0.0, byte0=1)], angles=[0.0])  # (5,0) -> 0 < 1
BLURRED["rounding constant"] = (im // 128).astype(np.uint8)
