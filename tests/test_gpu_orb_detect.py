"""GPU: gl_orb_pyramid and gl_orb_detect (the irregular half of ORBextractor, orb_extractor.cpp) == the sequential model
tests/orb_detect_ref.py, bit for bit on every output: the hand-built cases of tests/orb_detect_cases.py, random scenes, one 752 x 480
eight-level stereo pair, the composite orb.extract and the hand-over into gl_stereo_matches and gl_track_frame_chain.  Every run also
checks the guard words behind the outputs and that the pyramid has not changed (tests/orb_detect_dev.py).  No tolerance anywhere."""
import functools

import numpy as np
import pytest

from tests import orb_detect_cases as cases
from tests import orb_detect_dev as dev
from tests import orb_detect_ref as ref
from tests import orb_dev, orb_ref, orb_scenes
from tests.gpu_helpers import stop_on_device_error  # noqa: F401

pytestmark = pytest.mark.gpu

CAP = 2048  # candidate slots per level for the small scenes


@functools.lru_cache(maxsize=None)
def small(seed, nlevels=4, size=(160, 120)):
    """a random scene's pyramid, made by the model"""
    return dev.register(("small", seed, nlevels, size), ref.pyramid(dev.scene(seed, size), nlevels))


def bound(levels, nfeatures):
    per = ref.features_per_level(nfeatures, len(levels))
    return sum(ref.level_bound(l.shape[1], l.shape[0], n) for l, n in zip(levels, per))


def check(gpu, keys, nfeatures, label, cand_cap=CAP, N=None, **kw):
    torch, ctx = gpu
    frames = [dev.IMAGES[k] for k in keys]
    N = max(bound(frames[0], nfeatures), 1) if N is None else N
    got = dev.run(torch, ctx, frames, nfeatures, N, cand_cap, **kw)
    want = dev.expected([dev.model(k, nfeatures, cand_cap, kw.get("ini_th", 20), kw.get("min_th", 7)) for k in keys], N, cand_cap)
    dev.same_bits(got, want, label)
    return got


# ---- the hand-built cases: alone, and each group as one batch in both orders
@pytest.mark.parametrize("name", sorted(cases.DETECT))
def test_case_alone(gpu, name):
    c = cases.DETECT[name]
    got = check(gpu, [dev.register(("case", name), c["levels"])], c["nfeatures"], name, cand_cap=c["cand_cap"], N=c.get("N"),
                ini_th=c.get("ini_th", 20), min_th=c.get("min_th", 7))
    cases.check_declared(name, {k: v[0] for k, v in got.items()})


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_cases_as_one_batch(gpu, order):
    for group, names in sorted(cases.detect_groups().items()):
        names = sorted(names, reverse=order == "descending")
        c = cases.DETECT[names[0]]
        check(gpu, [dev.register(("case", n), cases.DETECT[n]["levels"]) for n in names], c["nfeatures"], "group %s %s" % (group, order),
              cand_cap=c["cand_cap"], N=c.get("N"), ini_th=c.get("ini_th", 20), min_th=c.get("min_th", 7))


@pytest.mark.parametrize("name", sorted(cases.RESIZE))
def test_resize_case(gpu, name):
    torch, ctx = gpu
    c = cases.RESIZE[name]
    frames = dev.run_pyramid(torch, ctx, [c["image"]], c["nlevels"], scale_factor=c["scale_factor"])
    for l, want in enumerate(ref.pyramid(c["image"], c["nlevels"], c["scale_factor"])):
        assert np.array_equal(frames[0][l], want), (name, l)
    cases.check_declared_resize(name, frames[0])


# ---- random scenes against the model
@pytest.mark.parametrize("B", [1, 3, 64])
def test_random_scenes(gpu, B):
    keys = [small(100 + b) for b in range(B)]
    m = dev.model(keys[0], 300, CAP)
    assert m["stat"][0] > 500 and m["stat"][2] > 200 and all(m["level_count"][:4] > 0), m["stat"]
    check(gpu, keys, 300, "B = %d" % B)


@pytest.mark.parametrize("nfeatures", [0, 1, 40, 2000])
def test_feature_counts(gpu, nfeatures):
    """N_l of 0 and 1, a count the octree reaches in phase 2, and one it never reaches"""
    check(gpu, [small(7), small(8)], nfeatures, "nfeatures = %d" % nfeatures)


def test_low_contrast_scene_falls_back_per_cell(gpu):
    key = dev.register("weak", ref.pyramid(dev.scene(5, contrast=0.12), 3))
    m = dev.model(key, 200, CAP)
    assert 0 < m["stat"][1] < sum(len(ref.cells(l.shape[1], l.shape[0])[2]) for l in dev.IMAGES[key]), m["stat"]
    check(gpu, [key], 200, "cells redone at min_th beside cells that are not")


def test_stride_above_width_and_offset(gpu):
    check(gpu, [small(100), small(101)], 300, "stride = width + 13, 7 bytes in front", row_pad=13, lead=7)


def test_working_set_in_the_scratch_block(gpu):
    """16 384 candidate slots are 64 KB of permutations: above the LDS limit, the octree works in the main scratch block"""
    check(gpu, [small(100), small(101)], 300, "cand_cap 16 384", cand_cap=16384)


def test_pyramid_matches_the_model(gpu):
    torch, ctx = gpu
    images = [dev.scene(s, (161, 119)) for s in (1, 2, 3)]
    frames = dev.run_pyramid(torch, ctx, images, 5, row_pad=5, lead=3)
    for im, f in zip(images, frames):
        for l, want in enumerate(ref.pyramid(im, 5)):
            assert np.array_equal(f[l], want), l


# ---- level sizes at every tile edge of the new kernels: one 752 x 480 eight-level stereo pair
BIG_CAP = 8192


@functools.lru_cache(maxsize=None)
def big_pair():
    return tuple(dev.register(("big", s), ref.pyramid(dev.scene(s, (752, 480), grain=10), 8)) for s in (11, 12))


def test_stereo_pair_752x480(gpu):
    keys = big_pair()
    for k in keys:
        m = dev.model(k, 1000, BIG_CAP)
        assert 3000 <= m["cand_count"][0] <= BIG_CAP and m["stat"][3] == 0 and m["stat"][2] >= 1000, (m["cand_count"], m["stat"])
    check(gpu, keys, 1000, "752 x 480, 8 levels, nfeatures 1 000", cand_cap=BIG_CAP)
    check(gpu, keys, 2000, "752 x 480, 8 levels, nfeatures 2 000", cand_cap=BIG_CAP)


# ---- the composite and the hand-overs
def test_extract_is_the_three_calls_and_the_models_key_points_described(gpu):
    from gmmloc_amd import orb
    torch, ctx = gpu
    d = torch.device("cuda:0")
    images = [dev.scene(s, (200, 150)) for s in (21, 22)]
    pattern, blur_w = orb_scenes.PATTERN, orb_ref.default_blur(2.0)
    pat = torch.from_numpy(pattern).to(d)
    im = torch.from_numpy(np.stack(images)).to(d)
    pyr, det, des = orb.extract(ctx, im, pat, nfeatures=250, nlevels=4, cand_cap=CAP)
    ctx.synchronize()
    pyr2 = orb.build_pyramid(ctx, im, 4)
    det2 = orb.detect(ctx, pyr2, 250, cand_cap=CAP)
    des2 = orb.describe(ctx, det2["kp_xy"], det2["kp_oct"], pat, pyr2, n_kp=det2["n_kp"])
    ctx.synchronize()
    assert torch.equal(pyr.data, pyr2.data)
    for a, b in ((det, det2), (des, des2)):
        for k in a:
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    N = det["kp_oct"].shape[1]
    for b, image in enumerate(images):
        levels = ref.pyramid(image, 4)
        m = ref.detect(levels, 250, cand_cap=CAP)
        n = len(m["kp_oct"])
        assert n > 150 and int(det["n_kp"][b]) == n
        want = orb_ref.describe(levels, m["kp_xy"], m["kp_oct"], pattern, blur_w)
        assert all(orb_ref.trig_margin_ok(v) for v in want["angle"] if v >= 0)  # (else the device's and the host's libm could disagree)
        ref_out = orb_dev.expected([want], N)
        got = {k: des[k][b:b + 1].cpu().numpy() for k in orb_dev.OUT_KEYS}
        orb_dev.same_bits(got, ref_out, "image %d described" % b)


def test_outputs_feed_the_stereo_matcher_and_the_chain(gpu):
    """orb.extract on a stereo pair, its arrays passed on without a copy: gl_stereo_matches and gl_track_frame_chain give the bits they
    give on the MODEL's arrays uploaded"""
    from gmmloc_amd import api, orb, stereo, synth
    from tests.test_gpu_chain import TH_LOCAL, TH_MM, pack
    torch, ctx = gpu
    d = torch.device("cuda:0")
    left = dev.scene(31, (240, 160))
    right = np.roll(left, -6, axis=1)
    pat = torch.from_numpy(orb_scenes.PATTERN).to(d)
    pyr, det, made = orb.extract(ctx, torch.from_numpy(np.stack([left, right])).to(d), pat, nfeatures=120, nlevels=3, cand_cap=CAP)
    ctx.synchronize()
    N = det["kp_oct"].shape[1]
    sides = []
    for image in (left, right):
        levels = ref.pyramid(image, 3)
        m = ref.detect(levels, 120, cand_cap=CAP)
        sides.append((levels, m, orb_ref.describe(levels, m["kp_xy"], m["kp_oct"], orb_scenes.PATTERN, orb_ref.default_blur(2.0))))
    models = orb_dev.expected([s[2] for s in sides], N)
    oct_np = np.full((2, N), -1, np.int32)
    for b, s in enumerate(sides):
        oct_np[b, :len(s[1]["kp_oct"])] = s[1]["kp_oct"]
    n_np = np.array([len(s[1]["kp_oct"]) for s in sides], np.int32)
    assert np.array_equal(det["kp_oct"].cpu().numpy(), oct_np) and np.array_equal(det["n_kp"].cpu().numpy(), n_np)
    uploaded = {k: torch.from_numpy(models[k]).to(d) for k in ("desc", "angle", "uv32", "uv64")}
    oct_, n_kp = det["kp_oct"], det["n_kp"]
    pl, pr = stereo.Pyramid([sides[0][0]], d), stereo.Pyramid([sides[1][0]], d)

    def matches(x):
        r = stereo.stereo_matches(ctx, api.Camera(fx=400.0, fy=400.0, bf=40.0, height=160),
                                  dict(feat_uv=x["uv64"][0:1], feat_oct=oct_[0:1], feat_desc=x["desc"][0:1], n_left=n_kp[0:1]),
                                  dict(r_uv=x["uv32"][1:2], r_oct=oct_[1:2], r_desc=x["desc"][1:2], n_right=n_kp[1:2]), pl, pr)
        ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in r.items()}

    got, want = matches(made), matches(uploaded)
    assert want["stat"][0, 1] >= 20, want["stat"]  # the two sides' descriptors do match
    for k in want:
        assert np.array_equal(got[k], want[k]), k

    cam = api.Camera()
    packed = pack(torch, [synth.synth_chain_frame(N, 100, 300, 4800 + 7 * N + b, cam) for b in range(2)])

    def chain(x):
        out = api.track_frame_chain(ctx, cam, api.Params(), dict(packed, feat_desc=x["desc"], feat_angle=x["angle"], feat_uv=x["uv64"]), th_mm=TH_MM,
                                    th_local=TH_LOCAL)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    got, want = chain(made), chain(uploaded)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k


# ---- errors and determinism
def test_every_refused_call_writes_nothing(gpu):
    from gmmloc_amd import api, orb, stereo
    torch, ctx = gpu
    d = torch.device("cuda:0")
    levels = dev.IMAGES[small(100)]
    pyr = stereo.Pyramid([levels], d)
    need = bound(levels, 300)

    def outputs(N):
        o = {k: torch.full((1, N) + ((tr,) if tr else ()), 7, dtype=getattr(torch, dt), device=d) for k, (dt, tr, _) in dev.SLOT.items()}
        o.update(n_kp=torch.full((1,), 7, dtype=torch.int32, device=d), level_count=torch.full((1, 8), 7, dtype=torch.int32, device=d),
                 stat=torch.full((1, 4), 7, dtype=torch.int32, device=d))
        return o

    for N, kw, what in ((need - 1, {}, "sum of the levels' bounds"), (4097, {}, "GL_ORB_MAX"), (need, dict(min_th=0), "thresholds"),
                        (need, dict(ini_th=6), "thresholds"), (need, dict(cand_cap=0), "cand_cap"), (need, dict(cand_cap=65536), "cand_cap")):
        out = outputs(N)
        with pytest.raises(api.GLError, match=what):
            orb.detect(ctx, pyr, 300, N, out=out, **kw)
        ctx.synchronize()
        assert all(bool((v == 7).all()) for v in out.values()), what
    out = outputs(need)
    orb.detect(ctx, pyr, 300, need, cand_cap=CAP, out=out)  # the bound itself is accepted
    ctx.synchronize()
    assert int(out["n_kp"][0]) == len(dev.model(small(100), 300, CAP)["kp_oct"])
    # the pyramid: level sizes that are not the rule's, and levels that overlap
    im = torch.from_numpy(dev.scene(1)[None]).to(d)
    good = orb.build_pyramid(ctx, im, 4)
    ctx.synchronize()
    before = good.data.clone()
    for field, l, v in (("width", 2, good.c.width[2] + 1), ("height", 3, good.c.height[3] - 1), ("offset", 2, good.c.offset[1] + 5)):
        c = orb.pyramid_layout(160, 120, 4)
        c.data = good.data.data_ptr()
        getattr(c, field)[l] = v
        with pytest.raises(api.GLError, match="pyramid"):
            ctx.call(ctx.lib.gl_orb_pyramid, 1, c, 1.2)
    ctx.synchronize()
    assert torch.equal(good.data, before)


def test_two_runs_give_identical_bytes(gpu):
    torch, ctx = gpu
    keys = [small(100), small(101), small(102)]
    runs = [dev.run(torch, ctx, [dev.IMAGES[k] for k in keys], 300, 400, CAP) for _ in range(2)]
    for k in dev.KEYS:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k


def test_host_tables_match_the_model(gpu):
    from gmmloc_amd import orb
    for nf in (0, 1, 500, 1000, 1200, 2000):
        for nl in (1, 4, 8):
            assert orb.features_per_level(nf, nl) == ref.features_per_level(nf, nl), (nf, nl)
    for w, h in ((752, 480), (640, 480), (1241, 376), (100, 101), (125, 75), (63, 63)):
        c = orb.pyramid_layout(w, h, 8)
        assert [(c.height[l], c.width[l]) for l in range(8)] == ref.level_sizes(w, h, 8), (w, h)


def test_malformed_arguments_are_refused_with_nothing_written(gpu):
    """the rest of the header's list, through the C entry points: B < 1, a NULL required pointer, nlevels outside 1 .. 8, a level above
    32 767 px, frames that overlap.  (A level more than 1 024 times as wide as tall cannot be built below 32 768 px: no case.)"""
    import ctypes as C

    from gmmloc_amd import _lib, api, stereo
    torch, ctx = gpu
    d = torch.device("cuda:0")
    levels = dev.IMAGES[small(100)]
    pyr = stereo.Pyramid([levels, levels], d)
    before = pyr.data.clone()
    N = bound(levels, 300)
    kp_xy = torch.full((2, N, 2), 7, dtype=torch.int32, device=d)
    kp_oct = torch.full((2, N), 7, dtype=torch.int32, device=d)
    n_kp = torch.full((2,), 7, dtype=torch.int32, device=d)

    def out(**null):
        o = _lib.gl_orb_detect_out()
        o.kp_xy, o.kp_oct, o.n_kp = kp_xy.data_ptr(), kp_oct.data_ptr(), n_kp.data_ptr()
        for k in null:
            setattr(o, k, None)
        return o

    def changed(**fields):
        c = _lib.gl_image_pyramid.from_buffer_copy(pyr.c)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    def detect(B, c, o):
        ctx.call(ctx.lib.gl_orb_detect, B, N, C.byref(c), 300, 1.2, 20, 7, CAP, C.byref(o) if o is not None else None)

    for B, c, o in ((0, pyr.c, out()), (2, pyr.c, None), (2, pyr.c, out(kp_xy=1)), (2, pyr.c, out(kp_oct=1)), (2, pyr.c, out(n_kp=1)),
                    (2, changed(data=None), out()), (2, changed(nlevels=0), out()), (2, changed(nlevels=9), out()),
                    (2, changed(width=(0, 32768), stride=(0, 32768)), out()), (2, changed(height=(1, 0)), out()),
                    (2, changed(stride=(2, pyr.c.width[2] - 1)), out()), (2, changed(offset=(1, -1)), out())):
        with pytest.raises(api.GLError):
            detect(B, c, o)
    for B, c in ((0, pyr.c), (2, changed(data=None)), (2, changed(nlevels=9)), (2, changed(frame_stride=pyr.c.frame_stride - 1)),
                 (2, changed(width=(0, 32768), stride=(0, 32768)))):
        with pytest.raises(api.GLError):
            ctx.call(ctx.lib.gl_orb_pyramid, B, C.byref(c), 1.2)
    with pytest.raises(api.GLError, match="frames overlap"):
        ctx.call(ctx.lib.gl_orb_pyramid, 2, C.byref(changed(frame_stride=pyr.c.frame_stride - 1)), 1.2)
    ctx.call(ctx.lib.gl_orb_pyramid, 1, C.byref(changed(frame_stride=0)), 1.2)  # one frame: its stride is not read
    ctx.synchronize()
    assert torch.equal(pyr.data[1], before[1])
    assert bool((kp_xy == 7).all()) and bool((kp_oct == 7).all()) and bool((n_kp == 7).all())
