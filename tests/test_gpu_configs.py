"""GPU parity of every entry point that reads the camera, the parameters or the scale factor, under the non-default
configurations of tests/configs.py (ANISO: fx != fy, another image size, the two lambdas apart, a 1.25 pyramid, another neighbour
threshold; WIDE: another size and aspect, a large baseline term; NOSTR: the structure chi2 test off, the lambdas apart), crossed with
the launch-shape options that change the formulation or the summation shape.  The default configuration cannot tell fx from fy,
one lambda from the other, the 1.2 table from any other: tests/test_oracle_configs.py shows, on the oracle alone, that each such
mistake moves these outputs by at least 100 x the tolerances held here.

The tolerances are those of the default-configuration test of the same entry point; every oracle call gets the configuration's
parameters.  The frames are checked on the CPU (test_oracle_configs.py::test_gpu_frames_are_stable) to be frames on which the oracle
does not move under a permutation of its points, so nothing is excluded here."""
import numpy as np
import pytest

import gmmloc_amd
from gmmloc_amd import api, synth
from tests import chain_glue as G
from tests import configs
from tests.configs import ANISO, CONFIGS
from tests.gpu_helpers import T
from tests.test_gpu_pose import TOL_R, TOL_T, make_frames, pose_err
from tests.test_gpu_pose import run_gpu as run_pose
from tests.test_gpu_track import _run_track, oracle_track
from tests.test_oracle_configs import pose_frames, track_frames_of  # the frames the CPU file checks for stability

pytestmark = pytest.mark.gpu

cfgs = pytest.mark.parametrize("cfg", CONFIGS, ids=repr)


# ------------------------------------------------------------------ gl_optimize_current_pose
@cfgs
def test_optimize_current_pose(gpu, oracle, map_v1, gt_sync, opt, cfg):
    """pose_waves 1 / 4 / 8 x pose_regs 0 / 1 x pose_compact 0 / 1 on sparse 1 200-slot frames, and a batch of 1 560 frames (the
    one-wave shape): pose within 1e-6 m / 1e-6 rad of the oracle under the configuration's parameters, masks and counts equal.
    ANISO: the bits of a frame are the same on every shape of one pose_compact setting, in the large batch and alone."""
    mean, cov = map_v1
    cam, prm, oprm = cfg.camera(), cfg.params(), cfg.orc_params(oracle)
    frames = pose_frames(mean, cov, gt_sync, cfg)
    ref = [oracle.optimize_current_pose(cam, f["pose_init"], f["Xw"], f["obs"], f["octave"], prm=oprm) for f in frames]

    def check(res, what):
        pose, outl, nin = res
        for i, (f, (p_ref, o_ref, n_ref)) in enumerate(zip(frames, ref)):
            dt, dr = pose_err(pose[i], p_ref)
            assert dt < TOL_T and dr < TOL_R, (what, i, dt, dr)
            has = f["octave"] >= 0
            assert np.array_equal(outl[i][has], o_ref[has]) and nin[i] == n_ref, (what, i)
    for compact in (0, 1):
        opt("pose_compact", compact)
        first = None
        for regs in (1, 0):
            opt("pose_regs", regs)
            for waves in (1, 4, 8):
                opt("pose_waves", waves)
                res = run_pose(gpu, cam, prm, frames)
                check(res, (compact, regs, waves))
                first = first or res
                if cfg is ANISO:
                    for a, b in zip(first, res):
                        assert np.array_equal(a, b), (compact, regs, waves)
        opt("pose_regs", 1)
        opt("pose_waves", 0)
        big = run_pose(gpu, cam, prm, [frames[i % 6] for i in range(1560)])
        check([x[:6] for x in big], (compact, "batch"))
        check([x[-6:] for x in big], (compact, "batch end"))
        one = run_pose(gpu, cam, prm, frames[2:3])
        if cfg is ANISO:
            for a, b, c in zip(first, big, one):
                assert np.array_equal(a, b[:6]) and np.array_equal(a[2:3], c), compact


# ------------------------------------------------------------------ gl_track_frames
@cfgs
def test_track_frames(gpu, oracle, map_v1, gt_sync, opt, cfg):
    """ba_shape 0 / -1 / 1 x ba_persist 0 / 1 on frames of 2 000 points and of 300: chi2 exact, pose 1e-6, associations exact, points
    1e-6 (stereo) / 5e-6 - the assertions of test_track_frames_matches_oracle.  ANISO: the same bits on every shape."""
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm, oprm = cfg.camera(), cfg.params(), cfg.orc_params(oracle)
    g = api.GMM(ctx, mean, cov, params=cfg.params())
    h = oracle.gmm_create(mean, cov)
    for frames in track_frames_of(mean, cov, gt_sync, cfg):
        ref = [oracle_track(oracle, h, cam, f, prm=oprm) for f in frames]
        first = None
        for persist in (1, 0):
            opt("ba_persist", persist)
            for shape in (0, -1, 1):
                opt("ba_shape", shape)
                res = _run_track(torch, ctx, g, cam, prm, frames)
                pose, Xw, assoc, d2 = res
                for i, (f, (keep, p_ref, pts_ref, a_ref, idx0, d20)) in enumerate(zip(frames, ref)):
                    assert np.array_equal(d2[i][keep], d20)
                    dt, dr = pose_err(pose[i], p_ref)
                    assert dt < 1e-6 and dr < 1e-6, (shape, persist, i, dt, dr)
                    assert np.array_equal(assoc[i][keep], a_ref), (shape, persist, i, int((assoc[i][keep] != a_ref).sum()))
                    err = np.abs(Xw[i][keep] - pts_ref).max(1)
                    assert err[f["obs"][keep][:, 2] >= 0].max() < 1e-6 and err.max() < 5e-6, (shape, persist, i, err.max())
                    assert (assoc[i][f["octave"] < 0] == -1).all()
                first = first or res
                if cfg is ANISO:
                    for a, b, what in zip(first, res, ("pose", "points", "assoc", "chi2")):
                        assert np.array_equal(a, b, equal_nan=True), (shape, persist, what)
    oracle.gmm_destroy(h)


def test_track_frames_result_independent_of_batch_aniso(gpu, map_v1, gt_sync, opt):
    """test_track_frames_result_independent_of_batch under ANISO: alone, in a handful, inside a batch larger than the chip"""
    torch, ctx = gpu
    mean, cov = map_v1
    cfg = ANISO
    cam, prm = cfg.camera(), cfg.params()
    g = api.GMM(ctx, mean, cov, params=cfg.params())
    opt("ba_shape", -1)
    for M, B in [(300, 300), (2000, 280)]:
        frames = make_frames(mean, cov, gt_sync["V1_03_difficult"], cfg.camlike(), 6, M, 5000 + M, outlier_frac=0.08)
        frames = [frames[i % 6] for i in range(B)]
        big = _run_track(torch, ctx, g, cam, prm, frames)
        for sel in ([1], [0, 1, 2, 3, 4, 5], list(range(40))):
            small = _run_track(torch, ctx, g, cam, prm, frames, sel)
            for a, b, what in zip(big, small, ("pose", "points", "assoc", "chi2")):
                assert np.array_equal(a[sel], b, equal_nan=True), (M, len(sel), what)


# ------------------------------------------------------------------ gl_track_frames_anchored
@cfgs
def test_track_frames_anchored(gpu, oracle, map_v1, gt_sync, opt, cfg):
    """the prior edge, the fixed pose (ba_first_as_prior = 0) and two fixed observers on chip and packed (ba_fixed_pack 0 / 1):
    the assertions of test_track_frames_prior_matches_oracle / _fixed_first_keyframe / _fixed_observers_match_oracle"""
    from tests.test_gpu_anchor import add_fixed, dev, oracle_anchored
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm, oprm = cfg.camera(), cfg.params(), cfg.orc_params(oracle)
    camlike = cfg.camlike()
    g = api.GMM(ctx, mean, cov, params=cfg.params())
    h = oracle.gmm_create(mean, cov)
    F = 2
    frames = [add_fixed(f, camlike, F, 900 + i) for i, f in
              enumerate(make_frames(mean, cov, gt_sync["V1_01_easy"], camlike, 3, 500, 45, outlier_frac=0.05))]
    frames[2]["octave"][::5] = -1
    args = lambda: (dev(torch, frames, "pose_init"), dev(torch, frames, "Xw"), dev(torch, frames, "obs"), dev(torch, frames, "octave"))
    # the prior edge alone (frame 1 rides unanchored)
    flags = np.array([1, 0, 1], np.uint8)
    pose, Xw, obs, octv = args()
    assoc, _, _ = gmmloc_amd.track_frames_anchored(ctx, g, cam, prm, pose, Xw, obs, octv, prior=T(torch, flags))
    torch.cuda.synchronize()
    pose, Xw, assoc = pose.cpu().numpy(), Xw.cpu().numpy(), assoc.cpu().numpy()
    for i, f in enumerate(frames):
        keep, p_ref, pts_ref, a_ref, _ = oracle_anchored(oracle, h, cam, f, bool(flags[i]), 0, prm=oprm)
        dt, dr = pose_err(pose[i], p_ref)
        assert dt < 1e-6 and dr < 1e-6, ("prior", i, dt, dr)
        assert np.array_equal(assoc[i][keep], a_ref), ("prior", i)
        err = np.abs(Xw[i][keep] - pts_ref).max(1)
        assert err[f["obs"][keep][:, 2] >= 0].max() < 1e-6 and err.max() < 1e-5
    # the fixed pose
    prm0, oprm0 = cfg.params(ba_first_as_prior=0), cfg.orc_params(oracle, ba_first_as_prior=0)
    pose, Xw, obs, octv = args()
    pose0 = pose.clone()
    assoc, _, _ = gmmloc_amd.track_frames_anchored(ctx, g, cam, prm0, pose, Xw, obs, octv, prior=torch.ones(3, dtype=torch.uint8).cuda())
    torch.cuda.synchronize()
    assert torch.equal(pose, pose0)
    Xw, assoc = Xw.cpu().numpy(), assoc.cpu().numpy()
    for i, f in enumerate(frames):
        keep, p_ref, pts_ref, a_ref, _ = oracle_anchored(oracle, h, cam, f, True, 0, prm=oprm0)
        assert np.array_equal(assoc[i][keep], a_ref), ("fixed pose", i)
        err = np.abs(Xw[i][keep] - pts_ref).max(1)
        assert err[f["obs"][keep][:, 2] >= 0].max() < 1e-6 and err.max() < 1e-5
    # two fixed observers, with and without the prior, on chip and packed
    for prior in (0, 1):
        ref = [oracle_anchored(oracle, h, cam, f, bool(prior), F, prm=oprm) for f in frames]
        for pack in (0, 1):
            opt("ba_fixed_pack", pack)
            pose, Xw, obs, octv = args()
            assoc, _, fe = gmmloc_amd.track_frames_anchored(
                ctx, g, cam, prm, pose, Xw, obs, octv, prior=torch.full((3,), prior, dtype=torch.uint8).cuda(),
                fixed_pose=dev(torch, frames, "fixed_pose"), fixed_obs=dev(torch, frames, "fixed_obs"), fixed_oct=dev(torch, frames, "fixed_oct"),
                want_erase=True)
            torch.cuda.synchronize()
            pose, Xw, assoc, fe = pose.cpu().numpy(), Xw.cpu().numpy(), assoc.cpu().numpy(), fe.cpu().numpy()
            for i, (f, (keep, p_ref, pts_ref, a_ref, fe_ref)) in enumerate(zip(frames, ref)):
                dt, dr = pose_err(pose[i], p_ref)
                assert dt < 1e-6 and dr < 1e-6, (prior, pack, i, dt, dr)
                assert np.array_equal(assoc[i][keep], a_ref) and np.array_equal(fe[i][keep], fe_ref), (prior, pack, i)
                assert fe_ref.sum() > 0
                err = np.abs(Xw[i][keep] - pts_ref).max(1)
                well = (f["obs"][keep][:, 2] >= 0) | ((f["fixed_oct"][keep] >= 0) & ~fe_ref.astype(bool)).any(1)
                assert err[well].max() < 1e-6 and err.max() < 1e-5, (prior, pack, i, err[well].max(), err.max())
    oracle.gmm_destroy(h)


# ------------------------------------------------------------------ gl_joint_optimization
def ba_problems(oracle, h, mean, cov, gt, cfg, P, F, L, seeds):
    from tests.test_gpu_ba import make_ba_problem
    probs, assocs = [], []
    for s in seeds:
        p = make_ba_problem(mean, cov, gt, cfg.camlike(), P, F, L, s, s % 2 == 0)
        idx, d2 = oracle.associate3d(h, p["points"])
        probs.append(p)
        assocs.append(np.where(d2 <= 9.0, idx, -1).astype(np.int32))
    return probs, assocs


@cfgs
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_joint_optimization(gpu, oracle, map_v1, gt_sync, opt, cfg, mode):
    """bagen_mode 0 / 1 / 2 / 3 on a batch of three small windows (3 free + 1 fixed poses, ~500 observations), one window below
    3 000 observations (5 + 3 poses) and one above (8 + 4 poses, 1 000 points): test_gpu_ba.check with the configuration's parameters"""
    from tests.test_gpu_ba import check, run_gpu
    opt("bagen_mode", mode)
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm, oprm = cfg.camera(), cfg.params(), cfg.orc_params(oracle)
    g = api.GMM(ctx, mean, cov, params=cfg.params())
    h = oracle.gmm_create(mean, cov)
    for P, F, L, seeds, lo, hi in ((3, 1, 150, (31, 32, 33), 0, 3000), (5, 3, 300, (50,), 0, 3000), (8, 4, 1000, (108,), 3000, 1 << 30)):
        probs, assocs = ba_problems(oracle, h, mean, cov, gt_sync["V1_01_easy"], cfg, P, F, L, seeds)
        assert all(lo <= len(p["obs_pose"]) < hi for p in probs), [len(p["obs_pose"]) for p in probs]
        out = run_gpu(gpu, g, cam, prm, probs, assocs)
        check(probs, assocs, out, oracle, h, cam, prm=oprm)
    oracle.gmm_destroy(h)


def test_default_route_bits_do_not_depend_on_the_batch_size_aniso(gpu, oracle, map_v1, gt_sync, opt):
    """test_default_route_bits_do_not_depend_on_the_batch_size (small window) under ANISO: alone, among 8, among 9, among 20"""
    from tests.test_gpu_ba import check, run_gpu
    opt("bagen_mode", 0)
    torch, ctx = gpu
    mean, cov = map_v1
    cfg = ANISO
    cam, prm, oprm = cfg.camera(), cfg.params(), cfg.orc_params(oracle)
    g = api.GMM(ctx, mean, cov, params=cfg.params())
    h = oracle.gmm_create(mean, cov)
    probs, assocs = ba_problems(oracle, h, mean, cov, gt_sync["V1_02_medium"], cfg, 2, 1, 150, range(900, 920))
    NOBS = max(len(p["obs_pose"]) for p in probs)
    ref = run_gpu(gpu, g, cam, prm, probs[:1], assocs[:1], nobs=NOBS)
    check(probs[:1], assocs[:1], ref, oracle, h, cam, prm=oprm)
    for B in (8, 9, 20):
        out = run_gpu(gpu, g, cam, prm, probs[:B], assocs[:B], nobs=NOBS)
        for k in range(5):
            assert np.array_equal(out[k][0], ref[k][0]), (B, k)
    oracle.gmm_destroy(h)


# ------------------------------------------------------------------ gl_search2d
@cfgs
@pytest.mark.parametrize("threads,slot_lds", [(256, None), (1024, None), (256, 24), (1024, 24)])
def test_search2d(gpu, oracle, map_v1, gt_sync, opt, cfg, threads, slot_lds):
    """renderView + searchCorrespondence under the configuration's camera and image size, both block shapes, the accepted list in
    LDS and spilled: rendered ids in order and candidates exact (the assertions of test_search2d_matches_oracle)"""
    torch, ctx = gpu
    opt("view_threads", threads)
    if slot_lds:
        opt("view_slot_lds", slot_lds)
    mean, cov = map_v1
    cam = cfg.camera()
    g = api.GMM(ctx, mean, cov, params=cfg.params())
    h = oracle.gmm_create(mean, cov)
    B, N = 4, 400
    gt = gt_sync["V1_01_easy"]
    poses = np.stack([synth.gt_row_to_Tcw(gt[(7 + i * 131) % gt.shape[0]]) for i in range(B)])
    rng = np.random.default_rng(3)
    uv = np.stack([rng.uniform(0, cam.width, (B, N)), rng.uniform(0, cam.height, (B, N))], 2)
    cand, ncand, vids, nview = g.search2d(cam, T(torch, poses), T(torch, uv), None, k=5, view_cap=4096)
    torch.cuda.synchronize()
    cand, ncand, vids, nview = cand.cpu().numpy(), ncand.cpu().numpy(), vids.cpu().numpy(), nview.cpu().numpy()
    tot = 0
    for b in range(B):
        ids, m2, c2, dep = oracle.render_view(h, cam, poses[b])
        assert nview[b] == len(ids) and np.array_equal(vids[b][:len(ids)], ids) and (vids[b][len(ids):] == -1).all(), b
        c_ref, n_ref = oracle.search_correspondence(h, uv[b], 5)
        assert np.array_equal(ncand[b], n_ref) and np.array_equal(cand[b], c_ref), b
        tot += len(ids)
    assert tot > 50 * B
    oracle.gmm_destroy(h)


# ------------------------------------------------------------------ B1 / A8 / B2 / createMapPoints
@pytest.fixture(scope="module")
def world(map_v1, gt_sync):
    import numpy_ref as nr
    mean, cov = map_v1
    seq = gt_sync["V1_01_easy"]
    return dict(mean=mean, cov=cov, comps=nr.build_components(mean, cov), seq=seq,
                poses=np.stack([synth.gt_row_to_Tcw(seq[i]) for i in (50, 900, 2100)]))


def str_thresh(cfg):
    return float(np.float32(np.float32(cfg.prm["tri_str_thresh"]) * np.float32(cfg.prm["tri_lambda2"])))


@cfgs
def test_optimize_point(gpu, oracle, map_v1, world, cfg):
    """the assertions of test_optimize_point_matches_oracle on the inputs of test_oracle_configs.point_inputs (400 points, every 6th
    observed off its plane).  NOSTR: points whose structure chi2 is above the threshold are kept - the == 0 branch decides"""
    from tests.test_oracle_configs import point_inputs
    torch, ctx = gpu
    cam, prm, oprm = cfg.camera(), cfg.params(), cfg.orc_params(oracle)
    g = api.GMM(ctx, *map_v1, params=cfg.params())
    h = oracle.gmm_create(*map_v1)
    d = point_inputs(world, cfg, N=400)
    N, f = d["N"], d["f"]
    pose = np.tile(d["pose"], (N, 1))
    r_ref = oracle.optimize_point(h, cam, d["X0"], f["obs"], f["octave"], pose, d["comp"], d["pz"], prm=oprm)
    res, c2p, c2s, est = api.optimize_point(ctx, g, cam, prm, T(torch, d["X0"]), T(torch, f["obs"]), T(torch, f["octave"]), T(torch, pose),
                                            T(torch, d["comp"]), T(torch, d["pz"]))
    torch.cuda.synchronize()
    res = res.cpu().numpy()
    assert np.array_equal(res, r_ref[0])
    np.testing.assert_allclose(est.cpu().numpy(), r_ref[3], rtol=0, atol=1e-9)
    np.testing.assert_allclose(c2p.cpu().numpy(), r_ref[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(c2s.cpu().numpy(), r_ref[2], rtol=1e-8, atol=1e-10)
    assert 0 < r_ref[0].sum() < N
    over = r_ref[2] > str_thresh(cfg)
    if cfg.prm["tri_check_str_chi2"]:
        assert over.any() and not res[over].any()
    else:
        assert (res[over] == 1).sum() > 3 and (res[over] == 0).any()  # both outcomes among the points the test would have failed
    oracle.gmm_destroy(h)


@cfgs
def test_check_map_association(gpu, oracle, map_v1, world, cfg):
    """search2d -> checkMapAssociation as test_check_map_association_matches_oracle, the neighbour walk on the graph the GMM built
    at the configuration's neighbor_dist_thresh.  NOSTR: associations the structure chi2 test would have refused are made."""
    from tests.test_oracle_configs import point_inputs
    torch, ctx = gpu
    cam, prm, oprm = cfg.camera(), cfg.params(), cfg.orc_params(oracle)
    g = api.GMM(ctx, *map_v1, params=cfg.params())
    h = oracle.gmm_create(*map_v1)
    d = point_inputs(world, cfg, N=600)
    N, f = d["N"], d["f"]
    octv = f["octave"].copy()
    octv[::9] = -1
    pose = d["pose"][None]
    cand, ncand, _, _ = g.search2d(cam, T(torch, pose), T(torch, f["obs"][None, :, :2]), None, k=5)
    pts_d = T(torch, d["X0"][None])
    out = api.check_map_association(ctx, g, cam, prm, T(torch, pose), pts_d, T(torch, f["obs"][None]), T(torch, octv[None]), cand, ncand)
    torch.cuda.synchronize()
    out, pts_o, cand, ncand = out.cpu().numpy()[0], pts_d.cpu().numpy()[0], cand.cpu().numpy()[0], ncand.cpu().numpy()[0]
    oracle.render_view(h, cam, d["pose"])
    c_ref, n_ref = oracle.search_correspondence(h, f["obs"][:, :2].copy(), 5)
    assert np.array_equal(cand, c_ref) and np.array_equal(ncand, n_ref)
    keep = octv >= 0
    o_ref, p_ref = oracle.check_map_association(h, cam, d["pose"], d["X0"][keep], f["obs"][keep], octv[keep], c_ref[keep], n_ref[keep], prm=oprm)
    assert np.array_equal(out[keep], o_ref), int((out[keep] != o_ref).sum())
    np.testing.assert_allclose(pts_o[keep], p_ref, rtol=0, atol=1e-9)
    assert (out[~keep] == -1).all() and np.array_equal(pts_o[~keep], d["X0"][~keep])
    assert (o_ref >= 0).sum() > 50 and (o_ref < 0).sum() > 10
    if not cfg.prm["tri_check_str_chi2"]:
        h2 = oracle.gmm_create(*map_v1)
        o_on, p_on = oracle.check_map_association(h2, cam, d["pose"], d["X0"][keep], f["obs"][keep], octv[keep], c_ref[keep], n_ref[keep],
                                                  prm=cfg.orc_params(oracle, tri_check_str_chi2=1))
        oracle.gmm_destroy(h2)
        # the branch decides: another component, or a point the failed optimisation would have left where it was (the final
        # Mahalanobis gate of 9 refuses most components whose structure chi2 is above the threshold either way)
        assert ((o_ref != o_on) | (np.abs(p_ref - p_on).max(1) > 1e-6)).sum() >= 3
    oracle.gmm_destroy(h)


@cfgs
def test_optimize_triangulation(gpu, oracle, map_v1, world, cfg):
    """the assertions of test_optimize_triangulation_matches_oracle (components exact, points 1e-9).  NOSTR: components the
    structure chi2 test would have refused are taken."""
    from tests.test_oracle_configs import point_inputs
    torch, ctx = gpu
    cam, prm, oprm = cfg.camera(), cfg.params(), cfg.orc_params(oracle)
    g = api.GMM(ctx, *map_v1, params=cfg.params())
    h = oracle.gmm_create(*map_v1)
    d = point_inputs(world, cfg, N=400)
    N, f = d["N"], d["f"]
    n1, n2 = (d["cands"] >= 0).sum(1).astype(np.int32), (d["cands2"] >= 0).sum(1).astype(np.int32)
    p1, p2 = np.tile(d["pose"], (N, 1)), np.tile(d["pose2"], (N, 1))
    oct2 = np.random.default_rng(4).integers(0, 8, N).astype(np.int32)
    xd = T(torch, d["X0"])
    out = api.optimize_triangulation(ctx, g, cam, prm, xd, T(torch, p1), T(torch, d["uvr1"]), T(torch, f["octave"]), T(torch, p2), T(torch, d["uvr2"]),
                                     T(torch, oct2), T(torch, d["cands"]), T(torch, n1), T(torch, d["cands2"]), T(torch, n2))
    torch.cuda.synchronize()
    args = (d["X0"], p1, d["uvr1"], f["octave"], p2, d["uvr2"], oct2, d["cands"], n1, d["cands2"], n2)
    o_ref, x_ref = oracle.optimize_triangulation(h, cam, *args, prm=oprm)
    assert np.array_equal(out.cpu().numpy(), o_ref), int((out.cpu().numpy() != o_ref).sum())
    np.testing.assert_allclose(xd.cpu().numpy(), x_ref, rtol=0, atol=1e-9)
    assert 20 < (o_ref >= 0).sum() < N
    if not cfg.prm["tri_check_str_chi2"]:
        o_on, _ = oracle.optimize_triangulation(h, cam, *args, prm=cfg.orc_params(oracle, tri_check_str_chi2=1))
        assert (o_on != o_ref).sum() > 3
    oracle.gmm_destroy(h)


@cfgs
def test_create_map_points(gpu, oracle, map_v1, gt_sync, cfg):
    """the assertions of test_create_map_points_matches_oracle at the configured scale factor.  NOSTR: both outcomes of the branch."""
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm, oprm = cfg.camera(), cfg.params(), cfg.orc_params(oracle)
    g = api.GMM(ctx, mean, cov, params=cfg.params())
    h = oracle.gmm_create(mean, cov)
    gt = gt_sync["V1_01_easy"]
    m = synth.synth_tri_matches(mean, cov, synth.gt_row_to_Tcw(gt[900]), synth.gt_row_to_Tcw(gt[915]), cfg.camlike(), 600, 5)
    x_ref, t_ref, c_ref = oracle.create_map_points(h, cam, scale_factor=cfg.scale_factor, prm=oprm, **m)
    keys = ("pose1", "uvr1", "depth1", "oct1", "pose2", "uvr2", "depth2", "oct2", "cand1", "n1", "cand2", "n2")
    x, t, c = api.create_map_points(ctx, g, cam, prm, *[T(torch, m[k]) for k in keys], scale_factor=cfg.scale_factor)
    torch.cuda.synchronize()
    x, t, c = x.cpu().numpy(), t.cpu().numpy(), c.cpu().numpy()
    assert np.array_equal(t, t_ref), int((t != t_ref).sum())
    assert np.array_equal(c, c_ref), int((c != c_ref).sum())
    sane = np.linalg.norm(x_ref, axis=1) < 100.0
    assert sane.mean() > 0.98
    np.testing.assert_allclose(x[sane], x_ref[sane], rtol=0, atol=1e-8)
    assert (t_ref > 0).sum() > 50 and (t_ref == 0).sum() > 20 and len(set(t_ref.tolist())) >= 4
    if not cfg.prm["tri_check_str_chi2"]:
        _, t_on, c_on = oracle.create_map_points(h, cam, scale_factor=cfg.scale_factor, prm=cfg.orc_params(oracle, tri_check_str_chi2=1), **m)
        assert ((t_on != t_ref) | (c_on != c_ref)).sum() > 3
    oracle.gmm_destroy(h)


# ------------------------------------------------------------------ the matchers
@cfgs
@pytest.mark.parametrize("shape", [0, 1])   # batch shape / few-frames shape (descriptors in LDS)
@pytest.mark.parametrize("fuv", [True, False])
def test_search_by_projection(gpu, oracle, opt, cfg, shape, fuv):
    from tests.test_gpu_match import run_gpu
    torch, ctx = gpu
    opt("match_desc_lds", shape)
    W, H, sf = cfg.cam["width"], cfg.cam["height"], cfg.scale_factor
    for NF, NP, th in ((300, 200, 3.0), (1200, 800, 3.0), (1200, 1500, 5.0), (64, 1500, 3.0)):
        frames = [synth.synth_match_frame(NF, NP, 1000 * NF + 7 * b, width=W, height=H, scale_factor=sf, dup_frac=0.3, float_uv=fuv) for b in range(3)]
        m, n = run_gpu(torch, ctx, frames, th, scale_factor=sf)
        tot = 0
        for b, f in enumerate(frames):
            m_ref, n_ref = oracle.search_by_projection(th=th, scale_factor=sf, **f)
            assert n[b] == n_ref and np.array_equal(m[b], m_ref), (NF, NP, b, int(n[b]), n_ref, int((m[b] != m_ref).sum()))
            tot += n_ref
        assert tot > 20


@cfgs
def test_search_by_projection_frame(gpu, oracle, cfg):
    """frame-to-frame matching under the configured camera and scale factor, float and double key-point coordinates in one batch"""
    from tests.test_gpu_match import run_gpu_frame
    torch, ctx = gpu
    cam, camlike, sf = cfg.camera(), cfg.camlike(), cfg.scale_factor
    for NF, NL, th, motion, mono in ((1200, 900, 7.0, "forward", False), (1000, 1000, 14.0, "backward", False), (800, 800, 7.0, "none", True)):
        frames = [synth.synth_motion_frames(NF, NL, 77 * NF + b, camlike, motion, float_uv=b % 2 == 0) for b in range(4)]
        m, n = run_gpu_frame(torch, ctx, frames, th, mono, True, cam=cam, scale_factor=sf)
        tot = 0
        for b, f in enumerate(frames):
            m_ref, n_ref = oracle.search_by_projection_frame(camlike, th=th, mono=mono, check_orientation=True, scale_factor=sf, **f)
            assert n[b] == n_ref and np.array_equal(m[b], m_ref), (motion, b, int(n[b]), n_ref, int((m[b] != m_ref).sum()))
            tot += n_ref
        assert tot > 50


@cfgs
@pytest.mark.parametrize("coords", ["double", "float", "mixed", "float_records_off"])
def test_fuse_search(gpu, oracle, opt, cfg, coords):
    from tests.test_gpu_match import FUSE_KEYS, _pack_fuse
    torch, ctx = gpu
    cam, sf = cfg.camera(), cfg.scale_factor
    if coords == "float_records_off":
        opt("fuse_records", 0)
    fc = lambda i: coords.startswith("float") or (coords == "mixed" and i % 2 == 0)
    frames = [synth.synth_fuse_frame(NF, NP, 800 + i, width=cam.width, height=cam.height, scale_factor=sf, float_coords=fc(i))
              for i, (NF, NP) in enumerate(((300, 260), (1200, 1500), (2000, 3000), (40, 900), (700, 30), (5, 5)))]
    for th in (3.0, 5.0):
        bi, bd = api.fuse_search(ctx, cam, *_pack_fuse(torch, frames), th=th, scale_factor=sf)
        torch.cuda.synchronize()
        bi, bd = bi.cpu().numpy(), bd.cpu().numpy()
        tot = 0
        for b, f in enumerate(frames):
            ri, rd, n = oracle.fuse_search(f["width"], f["height"], *[f[k] for k in FUSE_KEYS], th=th, scale_factor=sf)
            npn = len(ri)
            assert np.array_equal(bi[b, :npn], ri) and np.array_equal(bd[b, :npn], rd), (b, th, int((bi[b, :npn] != ri).sum()))
            assert (bi[b, npn:] == -1).all()
            tot += n
        assert tot > 1000


@cfgs
def test_project_map_points_and_level_steps(gpu, oracle, cfg):
    """gl_project_map_points every output bit for bit at the configured camera and scale factor; gl_level_steps at that factor: at
    each step the oracle gives level L, one float above it L + 1, and the device agrees either side of every step"""
    from tests.test_gpu_match import _pack_project
    torch, ctx = gpu
    cam, sf = cfg.camera(), cfg.scale_factor
    frames = [synth.synth_project_frame(NP, 600 + i, cfg.camlike(), scale_factor=sf) for i, NP in enumerate((400, 3000, 1500, 40, 1, 2500))]
    st = api.level_steps(sf)
    r = np.stack([st, np.nextafter(st, np.float32(100))], 1).reshape(-1)
    P = np.tile([0.0, 0.0, 1.0], (14, 1))
    steps = dict(pose_cw=np.array([0, 0, 0, 1, 0, 0, 0], float), t_wc=np.zeros(3), pos=P, normal=P, max_dist=r, min_dist=np.full(14, 0.01, np.float32),
                 cand=np.ones(14, np.uint8))
    frames.append(steps)
    out = api.project_map_points(ctx, cam, *_pack_project(torch, frames), scale_factor=sf)
    torch.cuda.synchronize()
    out = [o.cpu().numpy() for o in out]
    tot = 0
    for b, f in enumerate(frames):
        ref = oracle.project_map_points(cam, scale_factor=sf, **f)
        n = len(f["cand"])
        for o, rr, name in zip(out, ref[:5], ("uvr", "level", "viewcos", "dist", "inview")):
            assert np.array_equal(o[b, :n], rr), (b, name, int((o[b, :n] != rr).sum()))
            assert (o[b, n:] == 0).all()
        tot += ref[5]
    assert tot > 1500
    assert out[1][-1, :14].tolist() == [v for L in range(7) for v in (L, L + 1)]


@cfgs
def test_search_local_points(gpu, oracle, cfg):
    """gl_search_local_points = projection + searchByProjection in one call, as test_search_local_points_chain_matches_oracle"""
    from tests.test_gpu_match import _pack_project
    torch, ctx = gpu
    cam, sf = cfg.camera(), cfg.scale_factor
    PK = ("pose_cw", "t_wc", "pos", "normal", "max_dist", "min_dist", "cand")
    sizes = ((900, 2500), (1200, 4000), (300, 700), (50, 3000), (1000, 60), (700, 1800), (1100, 2200), (400, 3500))
    frames = [synth.synth_local_points_frame(NF, NP, 3000 + i, cfg.camlike(), scale_factor=sf, float_uv=i % 3 != 0) for i, (NF, NP) in enumerate(sizes)]
    B, NF, NP = len(frames), max(len(f["feat_oct"]) for f in frames), max(len(f["cand"]) for f in frames)
    t = dict(feat_uv=np.zeros((B, NF, 2)), feat_ur=np.full((B, NF), -1.0, np.float32), feat_oct=np.full((B, NF), -1, np.int32),
             feat_desc=np.zeros((B, NF, 32), np.uint8), feat_taken=np.zeros((B, NF), np.uint8), mp_desc=np.zeros((B, NP, 32), np.uint8))
    for b, f in enumerate(frames):
        for k in ("feat_uv", "feat_ur", "feat_oct", "feat_desc", "feat_taken"):
            t[k][b, :len(f["feat_oct"])] = f[k]
        t["mp_desc"][b, :len(f["cand"])] = f["mp_desc"]
    proj = _pack_project(torch, frames)
    tot = 0
    for th in (3.0, 5.0):
        match, nm, inview = api.search_local_points(ctx, cam, T(torch, t["feat_uv"]), T(torch, t["feat_ur"]), T(torch, t["feat_oct"]), T(torch, t["feat_desc"]),
                                                    T(torch, t["feat_taken"]), *proj, T(torch, t["mp_desc"]), th=th, scale_factor=sf)
        torch.cuda.synchronize()
        match, nm, inview = match.cpu().numpy(), nm.cpu().numpy(), inview.cpu().numpy()
        for b, f in enumerate(frames):
            uvr, lvl, vc, dd, iv, n = oracle.project_map_points(cam, scale_factor=sf, **{k: f[k] for k in PK})
            ref, nref = oracle.search_by_projection(cam.width, cam.height, f["feat_uv"], f["feat_ur"], f["feat_oct"], f["feat_desc"], f["feat_taken"],
                                                    uvr, lvl, vc, iv, f["mp_desc"], th=th, scale_factor=sf)
            nf, npn = len(ref), len(iv)
            assert np.array_equal(inview[b, :npn], iv) and (inview[b, npn:] == 0).all(), b
            assert np.array_equal(match[b, :nf], ref) and nm[b] == nref, (b, th, int((match[b, :nf] != ref).sum()))
            tot += nref
    assert tot > 1000, tot


@cfgs
def test_search_for_triangulation(gpu, oracle, cfg):
    from tests.test_gpu_match import _pack_pairs
    torch, ctx = gpu
    sf = cfg.scale_factor
    pairs = [synth.synth_tri_search_pair(N1, N2, 400 + i, cfg.camlike(), n_nodes=nodes, pad=1)
             for i, (N1, N2, nodes) in enumerate(((300, 350, 60), (1200, 1100, 200), (700, 900, 25), (64, 70, 5), (2000, 1900, 300), (500, 40, 80)))]
    k1, k2, fm, ep = _pack_pairs(torch, pairs)
    for only_stereo in (False, True):
        match, nm = api.search_for_triangulation(ctx, k1, k2, fm, ep, only_stereo, True, scale_factor=sf)
        torch.cuda.synchronize()
        match, nm = match.cpu().numpy(), nm.cpu().numpy()
        total = 0
        for b, p in enumerate(pairs):
            m_ref, n_ref = oracle.search_for_triangulation(p["kf1"], p["kf2"], p["fmat"], p["epipole"], only_stereo, True, scale_factor=sf)
            n1 = len(m_ref)
            assert np.array_equal(match[b, :n1], m_ref) and (match[b, n1:] == -1).all() and nm[b] == n_ref, (b, int((match[b, :n1] != m_ref).sum()))
            total += n_ref
        assert total > 100


@pytest.mark.parametrize("what", [1, 2, 3])
def test_update_map_points_scale_factor(gpu, what):
    """gl_update_map_points at scale factor 1.25 (the distance band max_dist / min_dist is its power): bit for bit against
    tests/map_point_ref.py, and not the bytes of scale factor 1.2 where the band is written"""
    from tests.test_gpu_map_points import assert_same, mixed_map, run_both
    torch, ctx = gpu
    m = mixed_map(13, extra=2000)
    got, ref = run_both(torch, ctx, m, what=what, scale_factor=ANISO.scale_factor)
    assert_same(got, ref)
    got12, _ = run_both(torch, ctx, m, what=what, scale_factor=1.2)
    assert (got12["min_dist"].tobytes() != got["min_dist"].tobytes()) == bool(what & 2)


# ------------------------------------------------------------------ the chains
@cfgs
@pytest.mark.parametrize("fallback", [False, True])
def test_track_frame_chain(gpu, oracle, cfg, fallback):
    """gl_track_frame_chain, and _front + _back, under the configured camera, parameters and scale factor together, without and
    with the key-frame fallback buffers (one frame 10 degrees off its prediction): every stage exact on the inputs the device gave
    it, poses 1e-6 (tests/chain_glue.py::check_chain); the two halves give the bits of the one call"""
    from tests.test_gpu_chain import pack, run_chain
    from tests.chain_glue import TH_LOCAL, TH_MM
    torch, ctx = gpu
    cam, prm, oprm, sf = cfg.camera(), cfg.params(), cfg.orc_params(oracle), cfg.scale_factor
    kw = dict(NK=500) if fallback else {}
    frames = [synth.synth_chain_frame(700, 600, 1400, 5700 + b, cfg.camlike(), scale_factor=sf, temporal_frac=(0.2 if b == 2 else 0.0),
                                      pred_rot_deg=(10.0 if (b == 1 and fallback) else None), **kw) for b in range(3)]
    out = run_chain(torch, ctx, frames, cam, prm, sf)
    res = [G.check_chain(oracle, cam, f, out, b, prm=oprm, scale_factor=sf) for b, f in enumerate(frames)]
    assert [r["front"]["mode"] for r in res] == ([0, 1, 0] if fallback else [0, 0, 0])
    assert sum(r["n3"] for r in res) > 0
    a = pack(torch, frames)
    front = api.track_frame_chain_front(ctx, cam, prm, a, th_mm=TH_MM, scale_factor=sf)
    both = api.track_frame_chain_back(ctx, cam, prm, a, front, th_local=TH_LOCAL, nn_ratio=0.8, scale_factor=sf)
    torch.cuda.synchronize()
    for k in out:
        assert np.array_equal(both[k].cpu().numpy(), out[k]), k


@cfgs
def test_track_frame_chain_map(gpu, oracle, cfg):
    """gl_track_frame_chain_map under the configuration: check_chain on the one call's outputs with the local map the device made
    (test_chain_map_stages_equal_the_oracle_on_the_device_made_list)"""
    from tests import local_map_ref as R
    from tests import local_map_scenes as S
    from tests.test_gpu_local_map import run_map_chain
    torch, ctx = gpu
    cam, prm, oprm, sf = cfg.camera(), cfg.params(), cfg.orc_params(oracle), cfg.scale_factor
    frames, s, lists, KFcap, NPcap = S.chain_scene("all_valid", cam=cfg.camlike(), scale_factor=sf)
    out, ls = run_map_chain(torch, ctx, frames, s, lists, NPcap, cam=cam, prm=prm, scale_factor=sf)
    n3 = 0
    for b, f in enumerate(frames):
        g = dict(f)
        g.update(R.gather_local_map(s["map"], ls["local_mp"][b], ls["n_local_mp"][b], NPcap, s["last_mp"][b], s["kf_feat_mp"][b]))
        c = G.check_chain(oracle, cam, g, out, b, prm=oprm, scale_factor=sf)
        n3 += c["n3"]
    assert n3 > 0


# ------------------------------------------------------------------ the neighbour graph
def test_neighbour_graph_at_the_configured_threshold(gpu, oracle, map_v1):
    """k_nbs reads neighbor_dist_thresh from the gl_params the GMM captured at creation: the graph of a GMM created with ANISO's
    parameters (1.75) is the oracle's at 1.75 - and not the graph at 2.5 (the assertions of test_neighbour_graph_matches_oracle)"""
    torch, ctx = gpu
    mean, cov = map_v1
    g = api.GMM(ctx, mean, cov, params=ANISO.params())
    h = oracle.gmm_create(mean, cov)
    ptr, col, dist = oracle.neighbours(h, thresh=ANISO.prm["neighbor_dist_thresh"])
    assert np.array_equal(g.get(api.F_NBS_PTR), ptr)
    assert np.array_equal(g.get(api.F_NBS_IDX), col)
    np.testing.assert_allclose(g.get(api.F_NBS_DIST), dist, rtol=0, atol=1e-12)
    assert 1000 < len(col) < 16048
    oracle.gmm_destroy(h)


# ------------------------------------------------------------------ the local BA from the resident map
@cfgs
def test_joint_optimization_from_map(gpu, oracle, map_v1, gt_sync, cfg):
    """gl_ba_window_build -> gl_joint_optimization -> gl_ba_window_apply on the geometric scene made with the configured camera: the
    bits of api.joint_optimization on the uploaded window, which is within test_gpu_ba.check's tolerances of the oracle"""
    from tests import ba_window_ref as R
    from tests import ba_window_scenes as S
    from tests.test_gpu_ba import check
    from tests.gpu_helpers import to_dev
    from tests.test_gpu_ba_window import to_host
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm, oprm = cfg.camera(), cfg.params(), cfg.orc_params(oracle)
    m, ba, kf = S.geometric_scene(mean, cov, gt_sync["V1_01_easy"], cfg.camlike())
    w = R.window_vec(m, ba, kf)
    P, F, L, nobs = w["P"], w["F"], w["L"], w["nobs"]
    g = api.GMM(ctx, mean, cov, params=cfg.params())
    poses, points = T(torch, w["poses"][None]), T(torch, w["points"][None])
    dropped, erase, iters = api.joint_optimization(ctx, g, cam, prm, P, F, poses, T(torch, w["prior"][None]), points, T(torch, w["assoc"][None]),
                                                   T(torch, w["obs_ptr"][None]), T(torch, w["obs_pose"][None]), T(torch, w["obs_uvr"][None]),
                                                   T(torch, w["obs_oct"][None]))
    torch.cuda.synchronize()
    up = [x.cpu().numpy() for x in (poses, points, dropped, erase, iters)]
    h = oracle.gmm_create(mean, cov)
    prob = dict(P=P, F=F, poses=w["poses"], prior=w["prior"], points=w["points"], obs_ptr=w["obs_ptr"], obs_pose=w["obs_pose"], obs_uvr=w["obs_uvr"],
                obs_oct=w["obs_oct"])
    check([prob], [w["assoc"]], up, oracle, h, cam, prm=oprm)
    oracle.gmm_destroy(h)
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    r = api.joint_optimization_from_map(ctx, g, cam, prm, md, bd, kf, (P + 3, F + 3, L + 50, nobs + 100))
    torch.cuda.synchronize()
    assert (r["P"], r["F"], r["L"], r["nobs"]) == (P, F, L, nobs)
    s = to_host(r["slab"])
    assert s["poses"][0, :P + F].tobytes() == up[0][0].tobytes() and s["points"][0, :L].tobytes() == up[1][0].tobytes()
    assert np.array_equal(s["dropped"][0, :L], up[2][0]) and np.array_equal(s["erase"][0, :nobs], up[3][0]) and s["iters"][0] == up[4][0]


# ------------------------------------------------------------------ the C++ adapter
def test_cpp_adapter_aniso(gpu, map_v1, gt_sync, tmp_path):
    """tests/cpp/adapter_check.cpp with setCamera / params() of ANISO: the outputs of the Python host under the same configuration,
    bit for bit"""
    from tests.test_gpu_adapter import adapter_case
    adapter_case(gpu, map_v1, gt_sync, tmp_path, ANISO.camera(), ANISO.params())
