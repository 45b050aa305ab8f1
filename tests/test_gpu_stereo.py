"""GPU: gl_stereo_matches (Frame::computeStereoMatches, frame.cpp:179-349) == the sequential model tests/stereo_ref.py, bit for bit on
every output: the hand-built cases of tests/stereo_cases.py, random scenes, and the shapes at which the kernel takes another path.
Every run also checks the guard words behind the outputs and that no input changed (tests/stereo_dev.py).  No tolerance anywhere."""
import numpy as np
import pytest

from tests import stereo_cases, stereo_dev, stereo_ref, stereo_scenes
from tests.gpu_helpers import stop_on_device_error  # noqa: F401

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2, 3)  # scenes on which the MODEL meets what test_random_scene asks of a scene (checked on the CPU: test_stereo_ref.py)


def model(scene, key):
    return stereo_scenes.model_of(key, scene)


def check(gpu, scenes, keys, label, **kw):
    torch, ctx = gpu
    frames = [s["frame"] for s in scenes]
    got = stereo_dev.run(torch, ctx, scenes[0]["cam"], scenes[0]["scale_factor"], frames, **kw)
    ref = stereo_dev.expected([model(s, k) for s, k in zip(scenes, keys)], got["feat_ur"].shape[1])
    stereo_dev.same_bits(got, ref, label)
    return got


# ---- the hand-built cases: alone, as one batch in both orders, padded to 257 slots
@pytest.mark.parametrize("name", sorted(stereo_cases.CASES))
def test_case_alone(gpu, name):
    torch, ctx = gpu
    c = stereo_cases.CASES[name]
    got = stereo_dev.run(torch, ctx, stereo_cases.CAM, stereo_cases.SCALE, [c["frame"]])
    stereo_dev.same_bits(got, stereo_dev.expected([c["expect"]], got["feat_ur"].shape[1]), name)


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("slots", [None, 257])
def test_cases_as_one_batch(gpu, order, slots):
    torch, ctx = gpu
    names = sorted(stereo_cases.CASES, reverse=order == "descending")
    got = stereo_dev.run(torch, ctx, stereo_cases.CAM, stereo_cases.SCALE, [stereo_cases.CASES[n]["frame"] for n in names], NF=slots, NR=slots)
    ref = stereo_dev.expected([stereo_cases.CASES[n]["expect"] for n in names], got["feat_ur"].shape[1])
    stereo_dev.same_bits(got, ref, "the cases %s" % order)


# ---- random scenes against the model
@pytest.mark.parametrize("seed", SEEDS)
def test_random_scene(gpu, seed):
    scene = stereo_scenes.random_scene(seed)
    m = model(scene, ("random", seed))
    nf = len(m["sad"])
    assert (m["feat_depth"] > 0).sum() >= 0.4 * nf and m["stat"][2] >= 1 and all(m["dropped"][k] >= 1 for k in (261, 306, 325)), \
        "the scene of seed %d does not exercise the rules: %s %s" % (seed, m["stat"], m["dropped"])
    check(gpu, [scene], [("random", seed)], "seed %d" % seed)


# ---- shapes
def sized(nf, nr):
    big = max(nf, nr) >= 1024
    return stereo_scenes.random_scene(1000 + nf * 7 + nr, size=(320, 240) if big else (160, 120), nfeat=nf, nright=nr)


@pytest.mark.parametrize("nf,nr", [(1, 1), (63, 65), (64, 64), (65, 63), (256, 257), (257, 256), (1024, 1024), (4096, 4096), (1, 4096), (4096, 1)])
def test_feature_counts(gpu, nf, nr):
    check(gpu, [sized(nf, nr)], [("sized", nf, nr)], "NF %d, NR %d" % (nf, nr), counts=False)


def test_4097_is_refused_with_nothing_written(gpu):
    from gmmloc_amd import api, stereo
    torch, ctx = gpu
    scene = stereo_scenes.random_scene(0, nfeat=4)
    f = scene["frame"]
    for NF, NR in ((4097, 4), (4, 4097)):
        a, NF, NR = stereo_dev.pack([f], NF, NR)
        t = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
        dev = t["feat_oct"].device
        pl, pr = stereo.Pyramid([f["pyr_left"]], dev), stereo.Pyramid([f["pyr_right"]], dev)
        out = {k: torch.full((1, 4 if k == "stat" else NF), 7, dtype=torch.float32 if k in ("feat_ur", "feat_depth") else torch.int32, device=dev)
               for k in stereo_dev.OUT_KEYS}
        with pytest.raises(api.GLError, match="GL_STEREO_MATCH_MAX"):
            stereo.stereo_matches(ctx, api.Camera(fx=100.0, bf=40.0, height=120), {k: t[k] for k in ("feat_uv", "feat_oct", "feat_desc")},
                                  {k: t[k] for k in ("r_uv", "r_oct", "r_desc")}, pl, pr, out=out)
        ctx.synchronize()
        assert all(bool((v == 7).all()) for v in out.values())


def test_one_row_band_of_300_right_key_points(gpu):
    scene = stereo_scenes.random_scene(77, nlevels=1, nfeat=300, row=60)
    m = model(scene, "band300")
    assert m["stat"][1] >= 100
    check(gpu, [scene], ["band300"], "300 key-points in one band")


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1025])
def test_list_length_for_the_selection(gpu, n):
    """the median rule's list has exactly n entries: a feature joins the list whatever the other features do, so a prefix of a scene's
    features whose last feature is the n-th to join has a list of n"""
    full = stereo_scenes.random_scene(31, size=(320, 240), nfeat=1300)
    joined = np.flatnonzero(model(full, "list-full")["match_r"] >= 0)
    assert len(joined) >= 1025
    k = int(joined[n - 1]) + 1
    scene = dict(full, frame=dict(full["frame"], feat_uv=full["frame"]["feat_uv"][:k], feat_oct=full["frame"]["feat_oct"][:k],
                                  feat_desc=full["frame"]["feat_desc"][:k]))
    assert model(scene, ("list", n))["stat"][1] == n
    check(gpu, [scene], [("list", n)], "a list of %d" % n)


@pytest.mark.parametrize("B", [1, 3, 64])
def test_batches(gpu, B):
    scenes = [stereo_scenes.random_scene(200 + b, nfeat=40 + 3 * (b % 9)) for b in range(B)]
    check(gpu, scenes, [("batch", b) for b in range(B)], "B = %d" % B)


@pytest.mark.parametrize("nlevels", [1, 8])
def test_levels(gpu, nlevels):
    scene = stereo_scenes.random_scene(300 + nlevels, size=(320, 240), nlevels=nlevels, nfeat=200)
    m = model(scene, ("levels", nlevels))
    assert m["stat"][1] >= 50 and len(set(scene["frame"]["feat_oct"][m["match_r"] >= 0])) == nlevels
    check(gpu, [scene], [("levels", nlevels)], "%d levels" % nlevels)


def test_stride_above_width_and_offset(gpu):
    scenes = [stereo_scenes.random_scene(s) for s in SEEDS[:2]]
    check(gpu, scenes, [("random", s) for s in SEEDS[:2]], "stride = width + 13, 7 bytes in front", row_pad=13, lead=7)


# ---- hand-over: the two columns as they lie on the device are what the other calls read
def test_outputs_feed_temporal_points_and_the_chain(gpu):
    """feat_ur / feat_depth of gl_stereo_matches, passed on without a copy: create_temporal_points on the stereo scene's own features, and
    gl_track_frame_chain on two tiny frames of tests/test_gpu_chain.py with the device-made feat_ur in place of theirs, give the bits
    that the same calls give on the MODEL's arrays uploaded"""
    from gmmloc_amd import api, key_frame, stereo, synth
    from tests import key_frame_create_cases as cc
    from tests.test_gpu_chain import TH_LOCAL, TH_MM, pack
    torch, ctx = gpu
    NF, B = 120, 2
    scenes = [stereo_scenes.random_scene(s, nfeat=NF) for s in SEEDS[:B]]
    models = stereo_dev.expected([model(s, ("random", seed)) for s, seed in zip(scenes, SEEDS)], NF)
    a, _, _ = stereo_dev.pack([s["frame"] for s in scenes])
    t = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    dev = t["feat_oct"].device
    pl = stereo.Pyramid([s["frame"]["pyr_left"] for s in scenes], dev)
    pr = stereo.Pyramid([s["frame"]["pyr_right"] for s in scenes], dev)
    fx, bf, height = scenes[0]["cam"]
    made = stereo.stereo_matches(ctx, api.Camera(fx=fx, fy=fx, bf=bf, height=height), {k: t[k] for k in ("feat_uv", "feat_oct", "feat_desc")},
                                 {k: t[k] for k in ("r_uv", "r_oct", "r_desc")}, pl, pr)
    uploaded = {k: torch.from_numpy(models[k]).cuda() for k in ("feat_ur", "feat_depth")}
    assert (models["feat_depth"] > 0).sum() > 150

    cam = api.Camera()
    pose = torch.tensor([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]] * B, dtype=torch.float64, device=dev)
    outlier = torch.from_numpy((np.arange(B * NF).reshape(B, NF) % 5 == 2).astype(np.uint8)).cuda()

    def temporal(depth):
        last = {k: torch.from_numpy(np.stack([v] * B)).cuda() for k, v in cc.last_rows(NF).items()}
        fr = dict(pose=pose, feat_uv=t["feat_uv"], feat_depth=depth, feat_oct=t["feat_oct"], held=torch.zeros((B, NF), dtype=torch.uint8, device=dev),
                  last_outlier=outlier, feat_desc=t["feat_desc"])
        r = key_frame.create_temporal_points(ctx, cam, fr, last, 1e9)
        return {k: v.cpu().numpy() for k, v in dict(r, **last).items()}

    got, ref = temporal(made["feat_depth"]), temporal(uploaded["feat_depth"])
    assert int(got["n_temp"].sum()) > 150
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k

    frames = [synth.synth_chain_frame(NF, 100, 300, 4800 + 7 * NF + b, cam) for b in range(B)]
    packed = pack(torch, frames)

    def chain(ur):
        out = api.track_frame_chain(ctx, cam, api.Params(), dict(packed, feat_ur=ur), th_mm=TH_MM, th_local=TH_LOCAL)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    got, ref = chain(made["feat_ur"]), chain(uploaded["feat_ur"])
    for k in ref:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
