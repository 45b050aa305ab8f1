"""The four integer decisions of the chain's front (tracking.cpp:345, :352, :53, :65; :305 logs) on the device, each with a frame on
either side (tests/track_cases.py), against tests/track_ref.py - the reference's text as a sequential model, NOT the device restated:
through gl_track_frame_chain, through _front + _back, and through gl_track_frame_chain_map.  Counts, modes and every match / drop
list are exact; searchLocalPoints is exact from the device's own stage-2 pose; poses are within 1e-6.  The cases of one buffer layout
run as ONE batch, so neighbouring workgroups sit on different branches, and each frame of fewer than 20 matches again alone."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import local_map_ref as R
from tests import local_map_scenes as S
from tests import track_cases as TC
from tests import track_ref as T
from tests.test_gpu_chain import pack, run_chain
from tests.test_gpu_local_map import run_halves, run_map_chain

pytestmark = pytest.mark.gpu

CAM = api.Camera()
# name -> (the cases of ONE batch, with the key-frame's buffers)
LAYOUTS = {"fallback": (TC.WITH_FALLBACK, True), "no_fallback": (TC.NO_FALLBACK, False), "large_fallback": (TC.LARGE, True),
           "large_no_fallback": (TC.LARGE, False)}


def frames_of(oracle, layout):
    names, fb = LAYOUTS[layout]
    return names, [TC.frame(oracle, n, fb) for n in names]


def check_front(oracle, f, out, b, pose_key="pose_mm", final=False):
    """the front's outputs of frame b against the model -> the model's result (searchLocalPoints run from the DEVICE's pose)"""
    r = T.track(oracle, CAM, f, pose_mm=out[pose_key][b])
    fb = "kf_desc" in f
    assert out["counts"][b, 0] == r["n1"], "stage 1: matches"
    assert out["counts2"][b, 0] == r["ret_mm"], "what trackWithMotionModel returns"
    assert out["counts2"][b, 3] == r["mode"], "mode"
    assert out["counts"][b, 1] == r["ninl"], "stage 2 / 2b: inliers"
    assert np.array_equal(out["drop_src"][b], r["drop_src"]), "stage 2: dropped matches"
    assert np.abs(out[pose_key][b] - r["pose"]).max() < 1e-6, "stage 2 / 2b: pose"
    if fb:
        assert out["counts2"][b, 1] == r["nbow"] and out["counts2"][b, 2] == r["ret_kf"], "stage 2b: counts"
        assert np.array_equal(out["match_kf"][b], r["match_kf"]) and np.array_equal(out["drop_kf"][b], r["drop_kf"]), "stage 2b: matches"
    else:
        assert out["counts2"][b, 1] == 0 and out["counts2"][b, 2] == 0
    if not final:
        assert np.array_equal(out["match_last"][b], r["match_last"]), "stage 2: kept matches"
    if r["n1"] < 20:  # tracking.cpp:352: nothing optimised, nothing dropped, no map point marked as seen
        assert (out["drop_src"][b] == -1).all()
        if not fb:
            assert out[pose_key][b].tobytes() == np.asarray(f["pose_cw"], np.float64).tobytes(), "the pose of a frame :352 returned on"
            assert out["counts"][b, 1] == 0
            if not final:  # stage 1's matches, every one of them
                assert (out["match_last"][b] >= 0).sum() == out["counts"][b, 0]
        else:  # the pose checked above is trackKeyFrame's (from the LAST frame's pose, on the key-frame's matches alone: :309-312)
            assert out["counts2"][b, 3] != 0 and (out["match_last"][b] == -1).all()
            assert out["counts"][b, 1] + (out["drop_kf"][b] >= 0).sum() == out["counts2"][b, 1]
    return r


def check_back(oracle, f, out, b, r):
    """stages 3 and 4 of frame b from the device's stage-2 pose"""
    if r["mode"] == 2:  # tracking.cpp:70: the reference has returned
        return
    assert out["counts"][b, 2] == r["n3"] and np.array_equal(out["match_local"][b], r["match_local"]), "stage 3: matches"
    assert np.array_equal(out["inview"][b], r["inview"]), "stage 3: in-view flags"
    assert np.array_equal(out["match_last"][b], r["match_last_final"]), "final last-frame associations"
    Xw, obs, oc = T.pose_problem(f, r)
    pose4, outl4, ninl4 = oracle.optimize_current_pose(CAM, out["pose_mm"][b], Xw, obs, oc)
    assert np.abs(out["pose"][b] - pose4).max() < 1e-6, "stage 4: pose"
    assert out["counts"][b, 3] == ninl4, "stage 4: inliers"
    assert np.array_equal(out["outlier"][b][oc >= 0], outl4[oc >= 0]), "stage 4: outliers"


@pytest.fixture(scope="module")
def batches(gpu, oracle):
    """the one-call chain on every layout's batch with the default options, run once"""
    torch, ctx = gpu
    return {k: run_chain(torch, ctx, frames_of(oracle, k)[1]) for k in LAYOUTS}


@pytest.mark.parametrize("compact", [0, -1])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_chain_takes_every_branch_as_the_reference_does(gpu, oracle, opt, layout, compact):
    torch, ctx = gpu
    opt("pose_compact", compact)
    names, frames = frames_of(oracle, layout)
    out = run_chain(torch, ctx, frames)
    for b, (n, f) in enumerate(zip(names, frames)):
        try:
            r = check_front(oracle, f, out, b, final=True)
            check_back(oracle, f, out, b, r)
        except AssertionError as e:
            raise AssertionError("%s (frame %d of %s, pose_compact %d): %s" % (n, b, layout, compact, e))
    if layout.startswith("large"):  # NF = 1 200 > 1 024 slots: the stage-4 problem of the trimmed frame is the compacted one
        assert frames[0]["feat_oct"].shape[0] > 1024


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_front_and_back_halves(gpu, oracle, batches, layout):
    """front: what the host reads for its bookkeeping (match_last as stage 2 left it, drop_src = the map points SEEN) equals the model;
    front + back: the bits of the one call"""
    torch, ctx = gpu
    prm = api.Params()
    names, frames = frames_of(oracle, layout)
    a = pack(torch, frames)
    front = api.track_frame_chain_front(ctx, CAM, prm, a, th_mm=float(T.TH_MM))
    torch.cuda.synchronize()
    fr = {k: v.cpu().numpy().copy() for k, v in front.items()}
    for b, (n, f) in enumerate(zip(names, frames)):
        try:
            check_front(oracle, f, fr, b, pose_key="pose")
        except AssertionError as e:
            raise AssertionError("%s (frame %d of %s): %s" % (n, b, layout, e))
    both = api.track_frame_chain_back(ctx, CAM, prm, a, front, th_local=float(T.TH_LOCAL), nn_ratio=0.8)
    torch.cuda.synchronize()
    for k, v in batches[layout].items():
        assert both[k].cpu().numpy().tobytes() == v.tobytes(), k


@pytest.mark.parametrize("layout", ["fallback", "no_fallback"])
def test_frame_below_20_alone_has_the_bits_of_the_batched_frame(gpu, oracle, batches, layout):
    torch, ctx = gpu
    names, frames = frames_of(oracle, layout)
    ran = 0
    for b, (n, f) in enumerate(zip(names, frames)):
        if n not in TC.BELOW_20:
            continue
        one = run_chain(torch, ctx, [f])
        r = check_front(oracle, f, one, 0, final=True)
        check_back(oracle, f, one, 0, r)
        for k, v in batches[layout].items():
            assert one[k][0].tobytes() == v[b].tobytes(), (n, k)
        ran += 1
    assert ran >= 6


def test_chain_map_takes_the_branches_as_the_reference_does(gpu, oracle):
    """gl_track_frame_chain_map on a scene with a frame of 19 matches whose would-be optimisation has outliers, a frame whose
    trackWithMotionModel returns 9 and one that tracks: the bits of front -> host updateLocalMap -> back, and - on the local map the
    DEVICE listed, gathered on the host - the model's decisions, lists and searchLocalPoints"""
    torch, ctx = gpu
    frames, s, lists, KFcap, NPcap = S.chain_scene("branches")
    out, ls = run_map_chain(torch, ctx, frames, s, lists, NPcap)
    ref, lr, _ = run_halves(torch, ctx, frames, s, lists, NPcap)
    for k in ref:
        if k in out:
            assert out[k].tobytes() == ref[k].tobytes(), k
    assert all(np.array_equal(ls[k], lr[k]) for k in lr)
    assert out["counts2"][:, 3].tolist() == S.CHAIN_MODES["branches"]
    assert out["counts"][0, 0] == 19 and (out["drop_src"][0] == -1).all() and out["counts2"][1, 0] == 9
    for b, f in enumerate(frames):
        g = dict(f)
        g.update(R.gather_local_map(s["map"], ls["local_mp"][b], ls["n_local_mp"][b], NPcap, s["last_mp"][b], s["kf_feat_mp"][b]))
        r = check_front(oracle, g, out, b, final=True)
        check_back(oracle, g, out, b, r)
