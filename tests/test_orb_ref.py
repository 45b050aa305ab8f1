"""CPU: the sequential model of gl_orb_describe (tests/orb_ref.py) gives every DECLARED output of tests/orb_cases.py; a second,
vectorised statement of the call agrees with it on the cases and on random scenes; and every rule of the model, swapped for its
neighbour, changes at least one declared case - the cases can see each rule."""
import math

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from tests import orb_cases, orb_ref, orb_scenes

f32, f64 = np.float32, np.float64
EXACT = ("desc", "moments", "uv32", "uv64", "stat")
KEYS = EXACT + ("angle",)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run_case(c, fn=orb_ref.describe, **kw):
    g = orb_cases.GROUPS[c["group"]]
    return fn(c["levels"], c["kp_xy"], c["kp_oct"], g["pattern"], g["blur_w"], kp_angle=c["kp_angle"], **kw)


def meets(got, e):
    """the declared outputs of a case: the exact ones bit for bit, the angle exactly or within orb_ref.ANGLE_BOUND of atan2"""
    if not all(bits_equal(got[k], e[k]) for k in EXACT):
        return False
    for a, want, near in zip(got["angle"], e["angle"], e["angle_near"]):
        if not (a == want if np.isnan(near) else abs((float(a) - near + 180.0) % 360.0 - 180.0) <= orb_ref.ANGLE_BOUND):
            return False
    return True


@pytest.mark.parametrize("name", sorted(orb_cases.CASES))
def test_model_gives_the_declared_outputs(name):
    c = orb_cases.CASES[name]
    got = run_case(c)
    assert meets(got, c["expect"]), (name, {k: got[k] for k in KEYS})
    if name in orb_cases.BLURRED:
        assert bits_equal(orb_ref.blur(c["levels"][0], orb_cases.GROUPS[c["group"]]["blur_w"]), orb_cases.BLURRED[name])


def test_declared_tables():
    assert orb_ref.UMAX == orb_cases.UMAX  # :449-463 run as written gives the header's table (749 pixels: asserted in orb_ref)
    assert bits_equal(orb_ref.scale_table(1.2), np.array(orb_cases.SF, f32))
    init_config = [f32(1.0)]
    for _ in range(7):
        init_config.append(f32(init_config[-1] * f32(1.2)))
    assert [float(v) for v in init_config[:3]] == orb_cases.SF[:3] and float(init_config[3]) != orb_cases.SF[3]  # the header says they differ
    assert orb_ref.default_blur(2.0) == orb_cases.SIGMA2
    g = [math.exp(-i * i / 8.0) for i in range(4)]
    assert [round(256 * v / (g[0] + 2 * sum(g[1:])), 2) for v in g] == [55.32, 48.82, 33.56, 17.96]
    assert int(np.rint(13 * math.sqrt(2.0))) == 18 and orb_ref.EDGE_THRESHOLD - 1 == 18


def test_fast_atan2_stays_within_its_bound():
    rng = np.random.default_rng(0)
    worst = 0.0
    for y, x in rng.integers(-700000, 700001, (20000, 2)):
        if x or y:
            d = abs((float(orb_ref.fast_atan2(y, x)) - math.degrees(math.atan2(y, x)) + 180.0) % 360.0 - 180.0)
            worst = max(worst, d)
    assert 0.009 < worst <= orb_ref.ANGLE_BOUND, worst
    assert orb_ref.fast_atan2(0, 0) == 0.0


def test_generator_conditions():
    """b == 0.5f was found; the contraction case is one; every case's steering angle keeps the 2^-40 margin"""
    assert orb_ref.steer(orb_cases.HALF_ANGLE)[1] == f32(0.5)
    a, b = orb_ref.steer(orb_cases.CONTRACT_ANGLE)
    p = orb_cases.GROUPS["contract"]["pattern"]
    plain, fused = orb_ref.sample_offsets(p, a, b), orb_ref.sample_offsets(p, a, b, ("contract",))
    assert (plain[0][0], plain[1][0]) == (6, 10) and (fused[0][0], fused[1][0]) == (6, 11)
    for name, c in orb_cases.CASES.items():
        for ang in run_case(c)["angle"]:
            assert ang == -1.0 or orb_ref.trig_margin_ok(ang), (name, ang)


def test_cases_cover_the_issues_list():
    assert len(orb_cases.CASES) >= 140
    shapes = {im.shape for c in orb_cases.CASES.values() for im in c["levels"]}
    assert shapes == {(39, 39), (48, 64)}


# ---- the second statement: all key-points of a level at once; the blur as a padded correlation, the patch as a mask over 31 x 31 windows
def fast_atan2_arrays(y, x):
    s = f32(f64(180.0) / f64(math.pi))
    p1, p3, p5, p7 = (f32(f32(c) * s) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
    ax, ay = np.abs(x), np.abs(y)
    c = np.minimum(ax, ay) / (np.maximum(ax, ay) + f32(orb_ref.DBL_EPSILON))
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(ay > ax, f32(90.0) - a, a)
    a = np.where(x < 0, f32(180.0) - a, a)
    return np.where(y < 0, f32(360.0) - a, a).astype(f32)


def vectorised(levels, kp_xy, kp_oct, pattern, blur_w, scale_factor=1.2, n_kp=None, kp_angle=None):
    n, nl = len(kp_oct), len(levels)
    n_kp = n if n_kp is None else min(max(int(n_kp), 0), n)
    H, W = np.array([im.shape[0] for im in levels]), np.array([im.shape[1] for im in levels])
    lc = np.clip(kp_oct, 0, nl - 1)
    x, y = kp_xy[:, 0].astype(np.int64), kp_xy[:, 1].astype(np.int64)
    ok = (np.arange(n) < n_kp) & (kp_oct >= 0) & (kp_oct < nl) & (x >= 19) & (x < W[lc] - 19) & (y >= 19) & (y < H[lc] - 19)
    taps = np.array([blur_w[3], blur_w[2], blur_w[1], blur_w[0], blur_w[1], blur_w[2], blur_w[3]], np.int64)
    V, U = np.mgrid[-15:16, -15:16]
    mask = np.abs(U) <= np.array(orb_cases.UMAX)[np.abs(V)]
    sf = np.ones(8, f32)
    for l in range(1, 8):
        sf[l] = f32(f64(sf[l - 1]) * f64(scale_factor))
    out = dict(desc=np.zeros((n, 32), np.uint8), angle=np.full(n, -1.0, f32), moments=np.zeros((n, 2), np.int32), uv32=np.full((n, 2), -1.0, f32))
    px, py = pattern[:, 0].astype(f32), pattern[:, 1].astype(f32)
    for l in range(nl):
        idx = np.flatnonzero(ok & (kp_oct == l))
        if not len(idx):
            continue
        img = levels[l].astype(np.int64)
        pad = np.pad(img, 3, mode="reflect")  # numpy's `reflect` does not repeat the edge: BORDER_REFLECT_101
        rows = sum(t * pad[:, j:j + img.shape[1]] for j, t in enumerate(taps))
        blurred = np.minimum((sum(t * rows[j:j + img.shape[0]] for j, t in enumerate(taps)) + 32768) >> 16, 255)
        if kp_angle is None:
            win = sliding_window_view(img, (31, 31))[y[idx] - 15, x[idx] - 15]
            m10, m01 = (win * (U * mask)).sum(axis=(1, 2)), (win * (V * mask)).sum(axis=(1, 2))
            out["moments"][idx] = np.stack([m10, m01], 1)
            ang = fast_atan2_arrays(m01.astype(f32), m10.astype(f32))
        else:
            ang = kp_angle[idx].astype(f32)
        out["angle"][idx] = ang
        rad = ang * orb_ref.FACTOR_PI
        a, b = np.cos(rad.astype(f64)).astype(f32)[:, None], np.sin(rad.astype(f64)).astype(f32)[:, None]
        r, c = np.rint(px[None] * b + py[None] * a).astype(np.int64), np.rint(px[None] * a - py[None] * b).astype(np.int64)
        t = blurred[y[idx, None] + r, x[idx, None] + c]
        out["desc"][idx] = np.packbits((t[:, 0::2] < t[:, 1::2]).reshape(len(idx), 32, 8), axis=2, bitorder="little").reshape(len(idx), 32)
        scale = sf[l] if l else f32(1.0)
        out["uv32"][idx] = np.stack([x[idx].astype(f32) * scale, y[idx].astype(f32) * scale], 1)
    out["uv64"] = out["uv32"].astype(f64)
    out["stat"] = np.array([ok.sum(), n_kp - ok.sum()], np.int32)
    return out


SCENES = {("random", s): dict(seed=s) for s in range(4)}
SCENES.update({("angles", 5): dict(seed=5, angles=True), ("levels", 8): dict(seed=308, size=(320, 240), nlevels=8, n=200),
               ("levels", 1): dict(seed=301, nlevels=1), ("count", 9): dict(seed=9, count=77)})


@pytest.mark.parametrize("key", list(SCENES), ids=str)
def test_vectorised_statement_agrees_on_scenes(key):
    scene = orb_scenes.random_scene(**SCENES[key])
    m, v = orb_scenes.model_of(key, scene), vectorised(**scene)
    assert m["stat"][0] >= 0.8 * m["stat"].sum() and m["stat"][1] >= 5  # the scene exercises the rules and the deviations
    for k in KEYS:
        assert bits_equal(v[k], m[k]), (key, k)


def test_vectorised_statement_agrees_on_the_cases():
    for name, c in orb_cases.CASES.items():
        m, v = run_case(c), run_case(c, fn=vectorised)
        for k in KEYS:
            assert bits_equal(v[k], m[k]), (name, k)


# A rule whose neighbour gives the same bits on EVERY input cannot be seen by any case; each with the reason:
UNOBSERVABLE = {}


@pytest.mark.parametrize("rule", orb_ref.MUTATIONS)
def test_each_rule_is_seen_by_a_case(rule):
    changed = [name for name, c in orb_cases.CASES.items() if not meets(run_case(c, mut=(rule,)), c["expect"])]
    if rule in UNOBSERVABLE:
        assert not changed, "%s is listed as unobservable (%s) but changes %s" % (rule, UNOBSERVABLE[rule], changed)
    else:
        assert changed, "no declared case sees the rule %s" % rule
