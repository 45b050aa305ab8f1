"""The sequential model of gl_orb_describe: the regular half of ORBextractor (orb_extractor.cpp), restated line by line with the rules
and the three deviations of include/gmmloc_hip.h.  Every float operation is one IEEE binary32 operation (numpy float32 scalars / arrays:
one rounding each, no contraction).  `mut`: names of rules swapped for their neighbour (tests/test_orb_ref.py shows the hand-built
cases see each).  Test infrastructure; nothing in the product imports it."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
HALF_PATCH_SIZE, EDGE_THRESHOLD = 15, 19  # :74-75
REACH = 13  # the largest pattern coordinate (deviation 3)
# the declared fastAtan2 against atan2, degrees: the polynomial itself errs by 0.009547 (at min = max; a 2 000 001-point grid in double),
# its float evaluation by at most five roundings of values below 360 (ulp 3.05e-5) more
ANGLE_BOUND = 0.0097
DBL_EPSILON = f64(2.0) ** -52
FACTOR_PI = f32(f64(3.1415926535897932384626433832795) / f64(f32(180.0)))  # :103, (float)(CV_PI / 180.f)

MUTATIONS = (["contract", "half_away", "reflect", "moments_blurred", "le", "blur_round", "swap_row_col"] +
             ["umax%+d@%d" % (d, v) for v in range(HALF_PATCH_SIZE + 1) for d in (-1, 1)])


def umax_table():
    """:449-463 as written"""
    umax = [0] * (HALF_PATCH_SIZE + 1)
    vmax = int(math.floor(f32(f32(HALF_PATCH_SIZE) * f32(math.sqrt(f32(2.0)))) / f32(2.0) + f32(1.0)))
    vmin = int(math.ceil(f32(f32(HALF_PATCH_SIZE) * f32(math.sqrt(f32(2.0)))) / f32(2.0)))
    hp2 = float(HALF_PATCH_SIZE * HALF_PATCH_SIZE)
    for v in range(vmax + 1):
        umax[v] = int(np.rint(math.sqrt(hp2 - v * v)))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


UMAX = umax_table()
assert UMAX == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3] and sum(2 * u + 1 for u in UMAX) * 2 - 31 == 749


def scale_table(scale_factor, nlevels=8):
    """mvScaleFactor (:413-416): a float times the extractor's DOUBLE scaleFactor, rounded to float"""
    sf = [f32(1.0)]
    for _ in range(1, nlevels):
        sf.append(f32(f64(sf[-1]) * f64(scale_factor)))
    return np.array(sf, f32)


def default_blur(sigma):
    """gl_orb_default_blur's declared rule"""
    g = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(4)]
    s = g[0] + 2.0 * (g[1] + g[2] + g[3])
    w = [0] + [int(np.rint(256.0 * (g[i] / s))) for i in range(1, 4)]
    w[0] = 256 - 2 * sum(w)
    return w


def border(i, n, mut=()):
    """BORDER_REFLECT_101 by index: -1 -> 1, n -> n - 2"""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        if "reflect" in mut:  # BORDER_REFLECT: -1 -> 0, n -> n - 1
            i = -i - 1 if i < 0 else 2 * n - 1 - i
        else:
            i = -i if i < 0 else 2 * n - 2 - i
    return i


def blur(img, w, mut=()):
    """:1029-1030 on the ROI alone: exact integer row pass, exact integer column pass, (s + 2^15) >> 16 saturated"""
    h, wd = img.shape
    taps = [(k, int(w[abs(k)])) for k in range(-3, 4)]
    src = img.astype(np.int64)
    row = sum(t * src[:, [border(x + k, wd, mut) for x in range(wd)]] for k, t in taps)   # r(x, y) = sum_k w[|k|] I(x + k, y)
    s = sum(t * row[[border(y + k, h, mut) for y in range(h)], :] for k, t in taps)       # s(x, y) = sum_k w[|k|] r(x, y + k)
    half = (1 << 15) - 1 if "blur_round" in mut else 1 << 15
    return np.minimum((s + half) >> 16, 255).astype(np.uint8)


def fast_atan2(y, x):
    """cv::fastAtan2 as the header declares it -> degrees, float32"""
    s = f32(f64(180.0) / f64(math.pi))
    p1, p3, p5, p7 = (f32(f32(c) * s) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
    x, y = f32(x), f32(y)
    ax, ay = abs(x), abs(y)
    eps = f32(DBL_EPSILON)
    if ax >= ay:
        c = f32(ay / f32(ax + eps))
    else:
        c = f32(ax / f32(ay + eps))
    c2 = f32(c * c)
    a = f32(f32(f32(f32(f32(f32(f32(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c)
    if ay > ax:
        a = f32(f32(90.0) - a)
    if x < 0:
        a = f32(f32(180.0) - a)
    if y < 0:
        a = f32(f32(360.0) - a)
    return a


def ic_angle(img, x, y, mut=()):
    """:77-101 -> (m_10, m_01, angle)"""
    umax = list(UMAX)
    for m in mut:
        if m.startswith("umax"):
            d, v = m[4:].split("@")
            umax[int(v)] += int(d)
    m_01 = m_10 = 0
    centre = img[y].astype(np.int64)
    for u in range(-umax[0], umax[0] + 1):                                 # :83-84 (umax[0] == HALF_PATCH_SIZE unless a mutation moves it)
        m_10 += u * int(centre[x + u])
    for v in range(1, HALF_PATCH_SIZE + 1):                                # :88-98, a row pair at a time
        d = umax[v]
        u = np.arange(-d, d + 1)
        val_plus, val_minus = img[y + v, x - d:x + d + 1].astype(np.int64), img[y - v, x - d:x + d + 1].astype(np.int64)
        m_10 += int((u * (val_plus + val_minus)).sum())
        m_01 += v * int((val_plus - val_minus).sum())
    return m_10, m_01, fast_atan2(f32(m_01), f32(m_10))                    # :100


def steer(angle):
    """the declared steering -> (a, b) float32: the correctly rounded float cosine and sine.  (:106-107 call libm's cosf / sinf, one float
    away at some angles: the header's `steering` row, tests/test_orb_ref_pin.py)"""
    rad = f32(f32(angle) * FACTOR_PI)
    return f32(math.cos(float(rad))), f32(math.sin(float(rad)))


def trig_margin_ok(angle, rel=2.0 ** -40):
    """the double cos / sin of the steering angle lie at least `rel` (relative) away from every float rounding boundary, so that no two
    correct-to-a-few-ulp libms can round them to different floats"""
    rad = float(f32(f32(angle) * FACTOR_PI))
    for v in (math.cos(rad), math.sin(rad)):
        r = f32(v)
        for nb in (np.nextafter(r, f32(np.inf)), np.nextafter(r, f32(-np.inf))):
            mid = (float(r) + float(nb)) / 2.0
            if abs(v - mid) < rel * abs(v):
                return False
    return True


def cv_round(v, mut=()):
    """cvRound of float32 values: half to even"""
    v = np.asarray(v, f32)
    if "half_away" in mut:
        return (np.sign(v) * np.floor(np.abs(v).astype(f64) + 0.5)).astype(np.int64)
    return np.rint(v).astype(np.int64)


def fma32(x, y, z):
    """fmaf for the magnitudes met here: the double product and sum are exact, so one rounding"""
    return (x.astype(f64) * y.astype(f64) + z.astype(f64)).astype(f32)


def sample_offsets(pattern, a, b, mut=()):
    """:112-114 for the 512 samples -> (row, column) relative to the key-point"""
    px, py = pattern[:, 0].astype(f32), pattern[:, 1].astype(f32)
    if "contract" in mut:  # x * b + y * a as fma(x, b, y * a), x * a - y * b as fma(x, a, -(y * b))
        r, c = fma32(px, np.full(512, b, f32), py * a), fma32(px, np.full(512, a, f32), -(py * b))
    else:
        r, c = px * b + py * a, px * a - py * b
    if "swap_row_col" in mut:
        r, c = c, r
    return cv_round(r, mut), cv_round(c, mut)


def orb_descriptor(blurred, x, y, angle, pattern, mut=(), ab=None):
    """computeOrbDescriptor (:104-147) -> 32 bytes.  ab: the steering (a, b) to use in place of steer(angle), as a host's libm gave it"""
    a, b = steer(angle) if ab is None else (f32(ab[0]), f32(ab[1]))
    row, col = sample_offsets(pattern, a, b, mut)
    t = blurred[y + row, x + col].astype(np.int64)                        # GET_VALUE(0 .. 511)
    t0, t1 = t[0::2], t[1::2]
    bits = (t0 <= t1) if "le" in mut else (t0 < t1)                        # bit j of byte i: the pair 16 i + 2 j (:116-143)
    return np.packbits(bits.reshape(32, 8), axis=1, bitorder="little").reshape(32)


def live(levels, x, y, oct_):
    """deviations 1 and 2"""
    if not 0 <= oct_ < len(levels):
        return False
    h, w = levels[oct_].shape
    return EDGE_THRESHOLD <= x <= w - 1 - EDGE_THRESHOLD and EDGE_THRESHOLD <= y <= h - 1 - EDGE_THRESHOLD


def describe(levels, kp_xy, kp_oct, pattern, blur_w, scale_factor=1.2, n_kp=None, kp_angle=None, mut=(), ab=None):
    """gl_orb_describe for ONE image: levels - its pyramid, 2-D uint8 arrays; kp_xy n x 2, kp_oct n; pattern 512 x 2 int8; blur_w 4 ints.
    ab: n x 2 float32, the steering of every slot in place of steer(angle) (tests/test_orb_ref_pin.py: the reference host's own).
    -> dict(desc, angle, moments, uv32, uv64, stat) with n rows."""
    assert np.abs(pattern).max() <= REACH, "deviation 3: the call refuses this pattern"
    n = len(kp_oct)
    n_kp = n if n_kp is None else min(max(int(n_kp), 0), n)
    sf = scale_table(scale_factor)
    out = dict(desc=np.zeros((n, 32), np.uint8), angle=np.full(n, -1.0, f32), moments=np.zeros((n, 2), np.int32), uv32=np.full((n, 2), -1.0, f32),
               uv64=np.full((n, 2), -1.0, f64), stat=np.zeros(2, np.int32))
    blurred = {}
    for i in range(n_kp):
        x, y, l = int(kp_xy[i, 0]), int(kp_xy[i, 1]), int(kp_oct[i])
        if not live(levels, x, y, l):
            out["stat"][1] += 1
            continue
        out["stat"][0] += 1
        if l not in blurred:
            blurred[l] = blur(levels[l], blur_w, mut)                      # :1029-1030
        if kp_angle is None:
            m_10, m_01, angle = ic_angle(blurred[l] if "moments_blurred" in mut else levels[l], x, y, mut)
            out["moments"][i] = (m_10, m_01)
        else:
            angle = f32(kp_angle[i])
        out["angle"][i] = angle
        out["desc"][i] = orb_descriptor(blurred[l], x, y, angle, pattern, mut, None if ab is None else ab[i])
        scale = sf[l] if l != 0 else f32(1.0)                              # :1039-1046
        out["uv32"][i] = (f32(f32(x) * scale), f32(f32(y) * scale))
        out["uv64"][i] = out["uv32"][i].astype(f64)
    return out
