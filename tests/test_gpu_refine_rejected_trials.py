"""The batch shape of the refine against the latency shape, for equal bits, and both against the oracle, on frames whose Levenberg path
is not the smooth one of the other tests.  The two shapes run the same per-point code, but the batch shape keeps a point's state in
its thread's LDS slot from pass to pass and from trial to trial - factors, backup, stale chi2, Huber weight - while a thread of the
latency shape owns one point: what a trial leaves behind in a slot and the next one must not pick up shows as a difference between
them.  (Written for a variant that carried {1 / z, rho, rho'} of an accepted trial in the free rows of the slot into the next
pass A; it was measured slower and is not in the tree - profiles/r18_carry_ab.txt -, the frames stand for whoever tries again.)
Frames on map_v1 at the strides where the canonical order changes (65: two chunks on one wave; 256; 257: two waves with unequal
slot counts; 2 000: eight waves, four slots), built so that a stage sees rejected AND accepted trials and every kind of point:
  * stereo and monocular observations;
  * a start pose 3 m off along the optical axis, so that the first Levenberg trials overshoot, are rejected and are followed by
    accepted ones (asserted from the trial and outer-iteration counters of set_stats_buffer);
  * points on a plane of the map whose observations come from 40 cm off that plane: the first gating round takes their GMM edge to
    level 1 (asserted: the device answers -1 for an association that passed the chi2 gate of the set-up);
  * observations 30 px off: the second gating round takes their reprojection edge to level 1, and the last stage runs them with
    the GMM edge alone (asserted on the oracle's erase flags: the entry point does not return them).
The reference's schedule (and the kernel's) only ever RAISES the level of an edge: no round takes one back to level 0.
Each case against the oracle at the tolerances of tests/test_gpu_track.py; one anchored call and one ba_step32 call, which take
other instances of the kernel."""
import numpy as np
import pytest

import gmmloc_amd
from gmmloc_amd import synth, api
from tests.test_gpu_anchor import oracle_anchored
from tests.test_gpu_pose import pose_err
from tests.test_gpu_track import oracle_track

pytestmark = pytest.mark.gpu

PUSH = 3.0  # m along the optical axis
OFF_PLANE = 0.4  # m; the edge goes to level 1 above 0.08 m (tri_str_thresh = 0.0064 m^2): where the observation is stronger than the plane the point ends the first stage beyond that


def build_frame(mean, cov, gt, cam, L, seed, push=PUSH):
    """synth.synth_frame (points drawn from the visible components, 15 % monocular, 8 % observations 30 px off) with, in every eighth
    slot, a point that sits ON its planar component while its observations come from OFF_PLANE beside it, and a start pose
    `push` metres off along the optical axis."""
    T = synth.gt_row_to_Tcw(gt[(seed * 37) % gt.shape[0]])
    f = synth.synth_frame(mean, cov, T, cam, L, seed, outlier_frac=0.08, mono_frac=0.15)
    rng = np.random.default_rng(seed + 7)
    R, t = synth.quat_to_R(T[:4]), T[4:]
    K = mean.shape[0]
    w, V = np.linalg.eigh(cov.reshape(K, 3, 3)[f["comp"]])
    lifted = np.zeros(L, bool)
    for l in range(3, L, 8):
        if not w[l, 0] < 1e-4:  # (not a degenerate component: no plane edge to gate)
            continue
        n = V[l, :, 0]
        x_obs = f["Xw"][l] + OFF_PLANE * n
        pc = R @ x_obs + t
        if pc[2] < 0.5 or abs((R @ n) @ pc) > 0.5 * np.linalg.norm(pc):  # (along the ray the plane is stronger than the disparity)
            continue
        sig = 0.3 * 1.2 ** f["octave"][l]
        u = cam.fx * pc[0] / pc[2] + cam.cx + rng.standard_normal() * sig
        v = cam.fy * pc[1] / pc[2] + cam.cy + rng.standard_normal() * sig
        ur = np.float64(np.float32(max(u - cam.bf / pc[2], 0.0)))
        f["obs"][l] = [u, v, ur]
        lifted[l] = True
    f["lifted"] = lifted
    f["pose_init"] = synth.perturb_pose(T, rng)
    f["pose_init"][6] += push  # every point `push` metres deeper: the first Gauss-Newton steps overshoot and are rejected
    return f


def run(torch, ctx, g, cam, prm, frames, prior=None):
    T = lambda key: torch.from_numpy(np.ascontiguousarray(np.stack([f[key] for f in frames]))).cuda()
    B = len(frames)
    pose, Xw = T("pose_init"), T("Xw")
    trials, outer = torch.zeros(B, dtype=torch.int32).cuda(), torch.zeros(B, dtype=torch.int32).cuda()
    ctx.set_stats_buffer(trials, outer)
    try:
        if prior is None:
            assoc, d2 = gmmloc_amd.track_frames(ctx, g, cam, prm, pose, Xw, T("obs"), T("octave"))
        else:
            assoc, d2, _ = gmmloc_amd.track_frames_anchored(ctx, g, cam, prm, pose, Xw, T("obs"), T("octave"),
                                                            prior=torch.from_numpy(np.asarray(prior, np.uint8)).cuda())
        torch.cuda.synchronize()
    finally:
        ctx.set_stats_buffer(None)
    return dict(pose=pose.cpu().numpy(), points=Xw.cpu().numpy(), assoc=assoc.cpu().numpy(), d2=d2.cpu().numpy(),
                trials=trials.cpu().numpy(), outer=outer.cpu().numpy())


def check_against_oracle(oracle, h, cam, frames, res, prior=None):
    """the comparison of test_track_frames_matches_oracle, with its tolerances; and the frame is what it was built to be"""
    for i, f in enumerate(frames):
        if prior is None:
            keep, p_ref, pts_ref, a_ref, idx0, d20 = oracle_track(oracle, h, cam, f)
            assert np.array_equal(res["d2"][i][keep], d20)
        else:
            keep, p_ref, pts_ref, a_ref, _ = oracle_anchored(oracle, h, cam, f, bool(prior[i]), 0)
        dt, dr = pose_err(res["pose"][i], p_ref)
        assert dt < 1e-6 and dr < 1e-6, (i, dt, dr)
        assert np.array_equal(res["assoc"][i][keep], a_ref), (i, int((res["assoc"][i][keep] != a_ref).sum()))
        err = np.abs(res["points"][i][keep] - pts_ref).max(1)
        stereo = f["obs"][keep][:, 2] >= 0
        assert err[stereo].max() < 1e-6 and err.max() < 5e-6, (i, int(np.argmax(err)), err.max())


def check_coverage(oracle, h, cam, f, res, i):
    """what the frame was built for did happen, on the device where it says so and on the oracle where it does not"""
    assert res["trials"][i] > res["outer"][i] > 0, ("no rejected trial", int(res["trials"][i]), int(res["outer"][i]))
    assert res["outer"][i] >= 6, "the stages stop at once: no accepted trial behind a rejected one"
    mono = f["obs"][:, 2] < 0
    assert mono.sum() > 0 and (~mono).sum() > 0
    gated_in = res["d2"][i] <= 9.0
    lost = gated_in & (res["assoc"][i] == -1)
    assert (lost & f["lifted"]).sum() > 0, "no GMM edge went to level 1"
    idx, d2 = oracle.associate3d(h, f["Xw"])
    a0 = np.where(d2 <= 9.0, idx, -1).astype(np.int32)
    L = len(a0)
    _, _, dropped, erase, _ = oracle.joint_optimization(h, cam, 1, 0, f["pose_init"][None], np.zeros(1, np.uint8), f["Xw"], a0,
                                                        np.arange(L + 1, dtype=np.int32), np.zeros(L, np.int32), f["obs"], f["octave"])
    gmm_only = (erase == 1) & (a0 >= 0) & (dropped == 0)
    assert gmm_only.sum() > 0, "no point ran the last stage on its GMM edge alone"
    assert ((erase == 1) & mono).sum() + ((erase == 1) & ~mono).sum() == (erase == 1).sum() > 0


# Seeds at which the oracle's own Levenberg trace (OG_TRACE, on the host) opens the first stage with three rejected trials - steps that
# overshoot, not rounding noise at the optimum - and accepts the ones behind them, and at which its final flags show at least one lifted
# point without its GMM edge and erased points that keep theirs.
SEEDS = {65: (196, 198), 256: (768, 769), 257: (771, 772), 2000: (6000,)}


@pytest.mark.parametrize("L", [65, 256, 257, 2000])
def test_shapes_agree_behind_rejected_trials(gpu, oracle, map_v1, gt_sync, opt, L):
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm = api.Camera(), api.Params()
    frames = [build_frame(mean, cov, gt_sync["V1_01_easy"], cam, L, seed) for seed in SEEDS[L]]
    g = api.GMM(ctx, mean, cov)
    h = oracle.gmm_create(mean, cov)
    res = {}
    for shape in (0, 1):  # the batch shape, the latency shape
        opt("ba_shape", shape)
        res[shape] = run(torch, ctx, g, cam, prm, frames)
    for what in ("pose", "points", "assoc", "trials", "outer"):
        assert res[0][what].tobytes() == res[1][what].tobytes(), (L, what)
    check_against_oracle(oracle, h, cam, frames, res[0])
    for i, f in enumerate(frames):
        check_coverage(oracle, h, cam, f, res[0], i)
    oracle.gmm_destroy(h)


def test_anchored_call_behind_rejected_trials(gpu, oracle, map_v1, gt_sync, opt):
    """the anchored instances; frame 1 rides unanchored in the same call, through the same instance"""
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm = api.Camera(), api.Params()
    frames = [build_frame(mean, cov, gt_sync["V1_01_easy"], cam, 257, 900 + i, push=1.0) for i in range(2)]
    g = api.GMM(ctx, mean, cov)
    h = oracle.gmm_create(mean, cov)
    prior = [1, 0]
    res = {}
    for shape in (0, 1):
        opt("ba_shape", shape)
        res[shape] = run(torch, ctx, g, cam, prm, frames, prior=prior)
    for what in ("pose", "points", "assoc"):
        assert res[0][what].tobytes() == res[1][what].tobytes(), what
    check_against_oracle(oracle, h, cam, frames, res[0], prior=prior)
    oracle.gmm_destroy(h)


def test_step32_call_behind_rejected_trials(gpu, oracle, map_v1, gt_sync, opt):
    """the fp32-step instances (their slot holds the fp32 cache instead of the factors).  Their step is not the exact one: both shapes
    are held to the oracle as test_track_frames_step32_option holds that option - the chi2 of the association exactly, the pose to 1e-4"""
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm = api.Camera(), api.Params()
    frames = [build_frame(mean, cov, gt_sync["V1_01_easy"], cam, 257, 950 + i, push=2.0) for i in range(2)]
    g = api.GMM(ctx, mean, cov)
    h = oracle.gmm_create(mean, cov)
    ref = [oracle_track(oracle, h, cam, f) for f in frames]
    opt("ba_step32", 1)
    for shape in (0, 1):
        opt("ba_shape", shape)
        res = run(torch, ctx, g, cam, prm, frames)
        for i, (keep, p_ref, pts_ref, a_ref, idx0, d20) in enumerate(ref):
            assert np.array_equal(res["d2"][i][keep], d20)
            dt, dr = pose_err(res["pose"][i], p_ref)
            assert dt < 1e-4 and dr < 1e-4, (shape, i, dt, dr)
    oracle.gmm_destroy(h)
