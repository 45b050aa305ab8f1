"""GPU: GL_ASSOC_SCREENED (fp32 screen + fp64 verify, gl_assoc32.hip) returns GL_ASSOC_EXHAUSTIVE's idx AND d2, bit for bit,
for every input - ordinary maps, adversarial maps and points, and every internal caller of the sweep under option
assoc_screen32 = 1 - and the counters show that the screen, not its fp64 fallback, does the work."""
import numpy as np
import pytest

import gmmloc_amd
from gmmloc_amd import synth, api
from tests.test_gpu_pose import make_frames
from tests.test_gpu_anchor import add_fixed, dev

pytestmark = pytest.mark.gpu

VER, FB = api.COUNTER_ASSOC_SCREEN_VERIFIED, api.COUNTER_ASSOC_SCREEN_FALLBACK


def _same(torch, g, pts, want_d2=True):
    """screened vs exhaustive on device points; returns (idx, d2) of the exhaustive run as numpy."""
    ie, de = g.associate3d(pts, api.ASSOC_EXHAUSTIVE, want_d2=want_d2)
    is_, ds = g.associate3d(pts, api.ASSOC_SCREENED, want_d2=want_d2)
    torch.cuda.synchronize()
    assert torch.equal(ie, is_), int((ie != is_).sum().item())
    if want_d2:
        assert torch.equal(de.isnan(), ds.isnan())
        assert torch.equal(torch.nan_to_num(de), torch.nan_to_num(ds))
        assert torch.equal(de.view(torch.int64), ds.view(torch.int64))  # bit for bit, signed zeros and infinities included
    return ie.cpu().numpy(), (de.cpu().numpy() if want_d2 else None)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_screened_synth_config2(gpu, seed):
    torch, ctx = gpu
    mean, cov = synth.synth_gmm(4096, seed)
    g = api.GMM(ctx, mean, cov)
    _same(torch, g, torch.from_numpy(synth.synth_points(mean, cov, 2000, seed)).cuda())
    if seed == 1:  # one batch of 2^20 points
        _same(torch, g, torch.from_numpy(synth.synth_points(mean, cov, 1 << 20, 77)).cuda())


@pytest.mark.parametrize("which", ["v1", "v2"])
def test_screened_real_maps(gpu, map_v1, map_v2, which):
    torch, ctx = gpu
    mean, cov = {"v1": map_v1, "v2": map_v2}[which]
    g = api.GMM(ctx, mean, cov)
    for N, seed in [(2000, 1), (1, 2), (63, 3), (257, 4), (30000, 5)]:
        _same(torch, g, torch.from_numpy(synth.synth_points(mean, cov, N, seed)).cuda())


def test_screened_config5(gpu):
    torch, ctx = gpu
    mean, cov = synth.synth_gmm(65536, 5)
    g = api.GMM(ctx, mean, cov)
    _same(torch, g, torch.from_numpy(synth.synth_points(mean, cov, 50000, 5)).cuda())


def _adversarial_map(K, seed):
    """anisotropy up to 1e8, a few huge and tiny components, duplicated components (exact ties)."""
    rng = np.random.default_rng(seed)
    mean, cov = synth.synth_gmm(K, seed)
    C = cov.reshape(K, 3, 3).copy()
    R = synth._haar(rng, 8)
    for j, lam in enumerate([(1e-8, 1.0, 1.0), (1e-6, 1e-6, 100.0), (1e-4, 1e-4, 1e-4), (1e-10, 1e-10, 1e-10),
                             (1e4, 1e4, 1e4), (100.0, 100.0, 1e-6), (1e-8, 1e-2, 1e-8), (2.0, 1e-8, 3.0)]):
        if j < K:
            C[j] = R[j] @ np.diag(lam) @ R[j].T
            C[j] = 0.5 * (C[j] + C[j].T)
    if K >= 24:  # exact duplicates: lowest index must win
        mean[16:20], C[16:20] = mean[4:8], C[4:8]
        mean[20:24], C[20:24] = mean[0:4], C[0:4]
    return mean, C.reshape(K, 9)


def _adversarial_points(mean, cov, N, seed):
    rng = np.random.default_rng(seed)
    K = mean.shape[0]
    pts = [synth.synth_points(mean, cov, N, seed)]
    pts.append(mean[: min(K, 64)])  # exactly on means
    if K >= 2:  # mirror-symmetric between two components: ulp-level near-ties
        a, b = rng.integers(0, K, 64), rng.integers(0, K, 64)
        pts.append(0.5 * (mean[a] + mean[b]))
        pts.append(0.5 * (mean[a] + mean[b]) + rng.standard_normal((64, 3)) * 1e-12)
    far = rng.standard_normal((8, 3))
    pts.append(1e6 * far / np.linalg.norm(far, axis=1, keepdims=True))  # 1e6 m outside the map
    pts.append(np.array([[1e30, 0.0, 0.0], [0.0, -1e30, 1.0]]))  # fp32 overflow
    pts.append(np.array([[np.nan, 0.0, 0.0], [1.0, np.inf, 0.0]]))  # NaN / inf coordinates
    return np.ascontiguousarray(np.concatenate(pts))


@pytest.mark.parametrize("K", [1, 17, 1000, 4099])
def test_screened_adversarial(gpu, K):
    torch, ctx = gpu
    mean, cov = _adversarial_map(K, 100 + K)
    g = api.GMM(ctx, mean, cov)
    pts = _adversarial_points(mean, cov, 3000, K)
    ctx.counter_read(FB)
    idx, d2 = _same(torch, g, torch.from_numpy(pts).cuda())
    assert ctx.counter_read(FB) > 0  # at least the 1e30 / NaN points took the fp64 sweep
    if K >= 24:
        on = min(K, 64)
        assert (idx[3000:3000 + on][16:24] < 16).all()  # the duplicates lose their ties
    # N = 1 and N = 0
    _same(torch, g, torch.from_numpy(pts[:1].copy()).cuda())
    e = torch.empty((0, 3), dtype=torch.float64, device="cuda")
    assert g.associate3d(e, api.ASSOC_SCREENED)[0].numel() == 0


def test_screened_nonfinite_map(gpu):
    """A map whose records fp32 cannot hold: every point goes through the fp64 sweep, same bits."""
    torch, ctx = gpu
    mean, cov = synth.synth_gmm(300, 9)
    cov[7] = np.diag([1e-41, 1.0, 1.0]).ravel()  # cov_inv 1e41: beyond fp32
    g = api.GMM(ctx, mean, cov)
    pts = torch.from_numpy(synth.synth_points(mean[:7], cov[:7], 500, 9)).cuda()
    ctx.counter_read(FB)
    _same(torch, g, pts)
    assert ctx.counter_read(FB) == 500


@pytest.mark.parametrize("which", ["synth", "adv"])
def test_screened_without_d2(gpu, which):
    torch, ctx = gpu
    mean, cov = synth.synth_gmm(4096, 2) if which == "synth" else _adversarial_map(1000, 3)
    g = api.GMM(ctx, mean, cov)
    pts = torch.from_numpy(_adversarial_points(mean, cov, 5000, 8)).cuda()
    idx, _ = _same(torch, g, pts, want_d2=True)
    i2, d2 = g.associate3d(pts, api.ASSOC_SCREENED, want_d2=False)
    assert d2 is None
    assert np.array_equal(i2.cpu().numpy(), idx)


def test_option_routes_index_remainder(gpu, opt):
    """GL_ASSOC_BRUTE through the cell index (assoc_index_min = 0): its unresolved points take the screened sweep."""
    torch, ctx = gpu
    mean, cov = synth.synth_gmm(4096, 1)
    g = api.GMM(ctx, mean, cov)
    assert g.index_info()["enabled"]
    pts = _adversarial_points(mean, cov, 20000, 3)
    pts = torch.from_numpy(np.ascontiguousarray(pts[np.abs(pts).max(1) < 100])).cuda()  # inside the index's grid
    opt("assoc_index_min", 0)
    ref = g.associate3d(pts, api.ASSOC_BRUTE)
    ctx.counter_read(VER)
    opt("assoc_screen32", 1)
    got = g.associate3d(pts, api.ASSOC_BRUTE)
    torch.cuda.synchronize()
    assert ctx.counter_read(VER) > 0  # the remainder went through the screen
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1].view(torch.int64), got[1].view(torch.int64))
    # and the small-problem sweep of GL_ASSOC_BRUTE (below assoc_index_min)
    opt("assoc_index_min", 1e12)
    got = g.associate3d(pts[:2000], api.ASSOC_BRUTE)
    opt("assoc_screen32", 0)
    ref = g.associate3d(pts[:2000], api.ASSOC_BRUTE)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1].view(torch.int64), got[1].view(torch.int64))


def _track(torch, ctx, g, cam, prm, frames, anchored, fixed):
    pose, Xw = dev(torch, frames, "pose_init"), dev(torch, frames, "Xw")
    obs, octv = dev(torch, frames, "obs"), dev(torch, frames, "octave")
    if not anchored:
        assoc, d2 = gmmloc_amd.track_frames(ctx, g, cam, prm, pose, Xw, obs, octv)
    elif fixed:
        pr = torch.ones((len(frames),), dtype=torch.uint8).cuda()
        assoc, d2, _ = gmmloc_amd.track_frames_anchored(ctx, g, cam, prm, pose, Xw, obs, octv, prior=pr,
                                                        fixed_pose=dev(torch, frames, "fixed_pose"),
                                                        fixed_obs=dev(torch, frames, "fixed_obs"),
                                                        fixed_oct=dev(torch, frames, "fixed_oct"))
    else:
        pr = torch.ones((len(frames),), dtype=torch.uint8).cuda()
        assoc, d2, _ = gmmloc_amd.track_frames_anchored(ctx, g, cam, prm, pose, Xw, obs, octv, prior=pr)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (pose, Xw, assoc, d2)]


@pytest.mark.parametrize("anchored,fixed", [(False, False), (True, False), (True, True)])
def test_option_track_frames_bit_identical(gpu, map_v1, gt_sync, opt, anchored, fixed):
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm = api.Camera(), api.Params()
    g = api.GMM(ctx, mean, cov)
    frames = make_frames(mean, cov, gt_sync["V1_01_easy"], cam, 6, 700, 321, outlier_frac=0.05)
    if fixed:
        frames = [add_fixed(f, cam, 2, 500 + i) for i, f in enumerate(frames)]
    opt("assoc_grid", 0)
    ref = _track(torch, ctx, g, cam, prm, frames, anchored, fixed)
    ctx.counter_read(VER)
    opt("assoc_screen32", 1)
    got = _track(torch, ctx, g, cam, prm, frames, anchored, fixed)
    assert ctx.counter_read(VER) > 0
    for a, b, what in zip(ref, got, ("pose", "points", "assoc", "d2")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def test_screen_counters_config2(gpu):
    """The screen does the work: few fp64 re-evaluations per point and almost no fallback on the config-2 map."""
    torch, ctx = gpu
    mean, cov = synth.synth_gmm(4096, 1)
    g = api.GMM(ctx, mean, cov)
    N = 2000 * 64
    pts = torch.from_numpy(synth.synth_points(mean, cov, N, 51)).cuda()
    ctx.counter_read(VER)
    ctx.counter_read(FB)
    g.associate3d(pts, api.ASSOC_SCREENED)
    ver, fb = ctx.counter_read(VER), ctx.counter_read(FB)
    assert ver >= N - fb
    assert ver / N < 4.0, ver / N
    assert fb / N < 0.01, fb / N
