"""GPU: gl_orb_describe (the regular half of ORBextractor, orb_extractor.cpp) == the sequential model tests/orb_ref.py, bit for bit on
every output: the hand-built cases of tests/orb_cases.py, random scenes with a seeded synthetic pattern, and the shapes at which the
kernels take another path.  Every run also checks the guard words behind the outputs and that no input changed (tests/orb_dev.py).
No tolerance anywhere: the generators keep the steering angles away from the float rounding boundaries of cos / sin (tests/orb_scenes.py,
tests/test_orb_ref.py)."""
import functools

import numpy as np
import pytest

from tests import orb_cases, orb_dev, orb_ref, orb_scenes
from tests.gpu_helpers import stop_on_device_error  # noqa: F401

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2, 3)
GROUPS = sorted(orb_cases.GROUPS)


@functools.lru_cache(maxsize=None)
def case_model(name):
    c = orb_cases.CASES[name]
    g = orb_cases.GROUPS[c["group"]]
    return orb_ref.describe(c["levels"], c["kp_xy"], c["kp_oct"], g["pattern"], g["blur_w"], kp_angle=c["kp_angle"])


def check(gpu, scenes, keys, label, **kw):
    """scenes of one pattern, blur and level shapes as ONE call against the model of each"""
    torch, ctx = gpu
    got = orb_dev.run(torch, ctx, scenes, scenes[0]["pattern"], scenes[0]["blur_w"], scenes[0]["scale_factor"], **kw)
    ref = orb_dev.expected([orb_scenes.model_of(k, s) for s, k in zip(scenes, keys)], got["angle"].shape[1])
    orb_dev.same_bits(got, ref, label)
    return got


# ---- the hand-built cases: alone, and each group's as one batch in both orders, padded to 257 slots
@pytest.mark.parametrize("name", sorted(orb_cases.CASES))
def test_case_alone(gpu, name):
    torch, ctx = gpu
    c = orb_cases.CASES[name]
    g = orb_cases.GROUPS[c["group"]]
    got = orb_dev.run(torch, ctx, [c], g["pattern"], g["blur_w"])
    orb_dev.same_bits(got, orb_dev.expected([case_model(name)], got["angle"].shape[1]), name)


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("slots", [None, 257])
def test_cases_as_one_batch(gpu, order, slots):
    torch, ctx = gpu
    for group in GROUPS:
        names = sorted((n for n, c in orb_cases.CASES.items() if c["group"] == group), reverse=order == "descending")
        g = orb_cases.GROUPS[group]
        got = orb_dev.run(torch, ctx, [orb_cases.CASES[n] for n in names], g["pattern"], g["blur_w"], N=slots)
        orb_dev.same_bits(got, orb_dev.expected([case_model(n) for n in names], got["angle"].shape[1]), "group %s %s" % (group, order))


# ---- random scenes against the model
@pytest.mark.parametrize("seed", SEEDS)
def test_random_scene(gpu, seed):
    scene = orb_scenes.random_scene(seed)
    m = orb_scenes.model_of(("random", seed), scene)
    assert m["stat"][0] >= 100 and m["stat"][1] >= 5 and len(set(scene["kp_oct"][m["angle"] >= 0])) == 3
    check(gpu, [scene], [("random", seed)], "seed %d" % seed)


def test_random_scene_with_given_angles_and_counts(gpu):
    scenes = [orb_scenes.random_scene(5, angles=True), orb_scenes.random_scene(6, angles=True, count=77)]
    check(gpu, scenes, [("angles", 5), ("angles-count", 6)], "kp_angle given, n_kp 120 and 77")


# ---- shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 4096])
def test_key_point_counts(gpu, n):
    check(gpu, [orb_scenes.random_scene(1000 + n, n=n)], [("sized", n)], "N = %d" % n, counts=False)


def test_4097_is_refused_with_nothing_written(gpu):
    from gmmloc_amd import api, orb, stereo
    torch, ctx = gpu
    scene = orb_scenes.random_scene(0, n=4)
    dev = torch.device("cuda:0")
    a, N = orb_dev.pack([scene], 4097)
    out = {k: torch.full((1, N) + ((tr,) if tr else ()), 7, dtype=getattr(torch, dt), device=dev) for k, (dt, tr, _) in orb_dev.OUT.items()}
    out["stat"] = torch.full((1, 2), 7, dtype=torch.int32, device=dev)
    with pytest.raises(api.GLError, match="GL_ORB_MAX"):
        orb.describe(ctx, torch.from_numpy(a["kp_xy"]).to(dev), torch.from_numpy(a["kp_oct"]).to(dev), torch.from_numpy(scene["pattern"]).to(dev),
                     stereo.Pyramid([scene["levels"]], dev), out=out)
    ctx.synchronize()
    assert all(bool((v == 7).all()) for v in out.values())


def test_bad_pattern_and_bad_weights_are_refused_with_nothing_written(gpu):
    from gmmloc_amd import api, orb, stereo
    torch, ctx = gpu
    scene = orb_scenes.random_scene(0, n=4)
    dev = torch.device("cuda:0")
    a, N = orb_dev.pack([scene])
    xy, oct_ = torch.from_numpy(a["kp_xy"]).to(dev), torch.from_numpy(a["kp_oct"]).to(dev)
    pyr = stereo.Pyramid([scene["levels"]], dev)
    good = torch.from_numpy(scene["pattern"]).to(dev)  # (stays alive: the bad pattern below is another buffer)
    out = {k: torch.full((1, N) + ((tr,) if tr else ()), 7, dtype=getattr(torch, dt), device=dev) for k, (dt, tr, _) in orb_dev.OUT.items()}
    out["stat"] = torch.full((1, 2), 7, dtype=torch.int32, device=dev)
    for entry in ((14, 0), (0, -14)):
        p = scene["pattern"].copy()
        p[300] = entry
        with pytest.raises(api.GLError, match="pattern entry"):
            orb.describe(ctx, xy, oct_, torch.from_numpy(p).to(dev), pyr, out=out)
    for w in ([54, 49, 34, -1], [0, 0, 0, 0], [255, 129, 0, 0]):  # a negative tap; sums of 0 and 513
        with pytest.raises(api.GLError, match="blur_w"):
            orb.describe(ctx, xy, oct_, good, pyr, blur_w=w, out=out)
    ctx.synchronize()
    assert all(bool((v == 7).all()) for v in out.values())
    assert orb.default_blur(2.0) == [54, 49, 34, 18] == orb_ref.default_blur(2.0)
    assert orb.default_blur(1.0) == orb_ref.default_blur(1.0) and orb.default_blur(3.5) == orb_ref.default_blur(3.5)


def test_taps_above_the_uint16_row_pass(gpu):
    """a tap sum above 257 takes the blur's 32-bit row pass; 512 is the largest"""
    scenes = [orb_scenes.random_scene(40, blur_w=w) for w in ([60, 50, 40, 9], [112, 100, 70, 30])]
    for s, w in zip(scenes, (258, 512)):
        assert s["blur_w"][0] + 2 * sum(s["blur_w"][1:]) == w
        check(gpu, [s], [("taps", w)], "taps summing to %d" % w)


@pytest.mark.parametrize("B", [1, 3, 64])
def test_batches(gpu, B):
    scenes = [orb_scenes.random_scene(200 + b, n=40 + 3 * (b % 9)) for b in range(B)]
    check(gpu, scenes, [("batch", b) for b in range(B)], "B = %d" % B)


@pytest.mark.parametrize("nlevels", [1, 8])
def test_levels(gpu, nlevels):
    scene = orb_scenes.random_scene(300 + nlevels, size=(320, 240), nlevels=nlevels, n=200)
    m = orb_scenes.model_of(("levels", nlevels), scene)
    assert len(set(scene["kp_oct"][m["angle"] >= 0])) == nlevels
    check(gpu, [scene], [("levels", nlevels)], "%d levels" % nlevels)


def test_stride_above_width_and_offset(gpu):
    scenes = [orb_scenes.random_scene(s) for s in SEEDS[:2]]
    check(gpu, scenes, [("random", s) for s in SEEDS[:2]], "stride = width + 13, 7 bytes in front", row_pad=13, lead=7)


@pytest.mark.parametrize("shape", [(39, 39), (48, 64), (65, 65), (97, 129)], ids=str)
def test_level_sizes_at_the_tile_edges(gpu, shape):
    """the blur's tiles are 64 x 32: one column / row less, exactly, and one more; 39 x 39 admits one key-point position"""
    scene = orb_scenes.random_scene(500 + shape[1], shapes=[shape], n=60)
    check(gpu, [scene], [("shape", shape)], "levels of %d x %d" % shape[::-1])


def test_a_level_too_small_for_key_points(gpu):
    """a level under 39 px admits no key-point and is not blurred; key-points that name it are skipped"""
    scene = orb_scenes.random_scene(700, shapes=[(48, 64), (30, 40)])
    scene["kp_oct"][::5] = 1
    scene["kp_xy"][::5] = (19, 10)
    m = orb_scenes.model_of("small-level", scene)
    assert m["stat"][0] >= 80 and m["stat"][1] >= 24
    check(gpu, [scene], ["small-level"], "a 40 x 30 level")


def test_a_level_without_key_points(gpu):
    scene = orb_scenes.random_scene(600, empty_level=1)
    assert 1 not in set(scene["kp_oct"])
    check(gpu, [scene], ["empty-level"], "no key-point on level 1")


# ---- hand-over: the arrays as they lie on the device are what the other calls read
def stereo_pair(seed, n):
    """a stereo scene of tests/stereo_scenes.py with key-points at level coordinates: the right ones where the texture went"""
    from tests import stereo_scenes
    s = stereo_scenes.random_scene(seed)
    left, right = s["frame"]["pyr_left"], s["frame"]["pyr_right"]
    shapes = [im.shape for im in left]
    base = orb_scenes.random_scene(seed, shapes=shapes, n=n, stray_every=10 ** 9)
    shift = np.array(stereo_scenes.SHIFT)[base["kp_oct"]]
    xy_l = base["kp_xy"].copy()
    xy_l[:, 0] = np.maximum(xy_l[:, 0], 19 + shift)
    xy_r = xy_l - np.stack([shift, np.zeros_like(shift)], 1)
    sides = [dict(base, levels=left, kp_xy=xy_l), dict(base, levels=right, kp_xy=xy_r.astype(np.int32))]
    return s, sides


def test_outputs_feed_the_stereo_matcher_and_the_chain(gpu):
    """desc / uv32 / uv64 / angle of gl_orb_describe, passed on without a copy: gl_stereo_matches on the device-made arrays of both sides,
    and gl_track_frame_chain on two tiny frames of tests/test_gpu_chain.py with the device-made feat_desc / feat_angle / feat_uv in
    place of theirs, give the bits that the same calls give on the MODEL's arrays uploaded"""
    from gmmloc_amd import api, orb, stereo, synth
    from tests.test_gpu_chain import TH_LOCAL, TH_MM, pack
    torch, ctx = gpu
    dev = torch.device("cuda:0")
    N = 120
    s, sides = stereo_pair(2, N)
    models = orb_dev.expected([orb_ref.describe(**side) for side in sides], N)
    assert all(orb_ref.trig_margin_ok(v) for v in models["angle"].ravel() if v >= 0)  # (the generator's condition, on the moved key-points too)
    a, _ = orb_dev.pack(sides)
    both = stereo.Pyramid([side["levels"] for side in sides], dev)
    made = orb.describe(ctx, torch.from_numpy(a["kp_xy"]).to(dev), torch.from_numpy(a["kp_oct"]).to(dev), torch.from_numpy(sides[0]["pattern"]).to(dev),
                        both, blur_w=sides[0]["blur_w"])
    uploaded = {k: torch.from_numpy(models[k]).to(dev) for k in ("desc", "angle", "uv32", "uv64")}
    oct_ = torch.from_numpy(a["kp_oct"]).to(dev)
    fx, bf, height = s["cam"]
    pl, pr = stereo.Pyramid([sides[0]["levels"]], dev), stereo.Pyramid([sides[1]["levels"]], dev)

    def matches(d):
        r = stereo.stereo_matches(ctx, api.Camera(fx=fx, fy=fx, bf=bf, height=height), dict(feat_uv=d["uv64"][0:1], feat_oct=oct_[0:1], feat_desc=d["desc"][0:1]),
                                  dict(r_uv=d["uv32"][1:2], r_oct=oct_[1:2], r_desc=d["desc"][1:2]), pl, pr)
        ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in r.items()}

    got, ref = matches(made), matches(uploaded)
    assert ref["stat"][0, 1] >= 30, ref["stat"]  # the descriptors of the two sides do match
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k

    cam = api.Camera()
    packed = pack(torch, [synth.synth_chain_frame(N, 100, 300, 4800 + 7 * N + b, cam) for b in range(2)])

    def chain(d):
        out = api.track_frame_chain(ctx, cam, api.Params(), dict(packed, feat_desc=d["desc"], feat_angle=d["angle"], feat_uv=d["uv64"]), th_mm=TH_MM,
                                    th_local=TH_LOCAL)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    got, ref = chain(made), chain(uploaded)
    for k in ref:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
