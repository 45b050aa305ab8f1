"""The batch refine keeps a thread's association indices in registers, 16 bits per point slot (gl_ba_fast_impl.hpp: AssocW), instead of
reading one from the launch's scratch at the head of every slot of every pass.  Frames built by hand so that the slots of ONE lane carry
different values - component 0, component K - 1, no association (gated out by chi2 > 9 in the refine's set-up, or handed over as -1 by
a call without the chi2 output), a non-degenerate component, a slot without a map point - at the sizes where the packing can go wrong, against the oracle as tests/test_gpu_track.py does, and the batch shape
against the latency shape (which never packs anything) for equal bits.  A map of more than 65 536 components takes the instances that
still load, an anchored call the anchored instances."""
import numpy as np
import pytest

import gmmloc_amd
from gmmloc_amd import synth, api
from tests.test_gpu_anchor import oracle_anchored
from tests.test_gpu_pose import pose_err
from tests.test_gpu_track import oracle_track

pytestmark = pytest.mark.gpu

EYE, TARGET = [0.0, 0.0, 0.9], [3.0, 0.0, 0.9]
BLOBS = np.array([[2.0, -0.8, 1.0], [2.2, 0.7, 1.2], [1.8, 0.15, 0.6]])


def _cov(normal, lam):
    """R diag(lam) R^T with the first axis along `normal`, bit-symmetric"""
    n = np.asarray(normal, float) / np.linalg.norm(normal)
    a = np.cross(n, [0.3, -0.5, 0.8])
    a /= np.linalg.norm(a)
    R = np.stack([n, a, np.cross(n, a)], 1)
    c = R @ np.diag(lam) @ R.T
    return 0.5 * (c + c.T)


def build_map(K, wall, floor, blobs, side):
    """K components: a wall x = 3 at index `wall`, a floor z = 0 at index `floor`, a side wall y = -1.2 at index `side` (planes:
    degenerate components; three of them, so that the structure holds the pose in every direction), three small volumes at the
    indices `blobs` (non-degenerate), every other component a small plane patch far behind the camera.  The component that
    shares the low 16 bits of a named index above 65 535 is a plane patch like any other: a wrong plane record would show."""
    rng = np.random.default_rng(K)
    mean = np.empty((K, 3))
    mean[:, 0] = -20.0 - 0.01 * np.arange(K)
    mean[:, 1:] = rng.uniform(-3.0, 3.0, (K, 2))
    cov = np.empty((K, 3, 3))
    cov[:] = _cov([1.0, 0.2, -0.1], [1e-6, 4e-3, 9e-3])
    mean[wall], cov[wall] = [3.0, 0.0, 1.2], _cov([1.0, 0.0, 0.0], [1e-6, 2.0, 1.5])
    mean[floor], cov[floor] = [2.5, 0.0, 0.0], _cov([0.0, 0.0, 1.0], [1e-6, 2.0, 1.8])
    mean[side], cov[side] = [2.4, -1.2, 1.0], _cov([0.0, 1.0, 0.0], [1e-6, 1.6, 1.2])
    for j, b in enumerate(blobs):
        mean[b], cov[b] = BLOBS[j], _cov([0.2 * j, 1.0, 0.5], [1.5e-3, 3e-3, 5e-3])
    return mean, np.ascontiguousarray(cov.reshape(K, 9))


def build_frame(mean, cov, cam, L, seed, wall, floor, blobs, side, empties):
    """A frame of L slots whose order k_ba1_prep keeps (points of planes and unassociated points first, in the caller's order, then the
    points of volumes, then the empty slots): point l of the first class is on the wall / on the floor / in free space, far from every
    component / on the side wall, by (chunk + l) % 4 - so the slots of a lane (chunks g, g + G, ...) differ; then max(2, L / 8) points in the
    volumes; then max(1, L / 16) slots without a map point when `empties`."""
    rng = np.random.default_rng(seed)
    nB, nE = max(2, L // 8), (max(1, L // 16) if empties else 0)
    nA = L - nB - nE
    X = np.empty((L, 3))
    kind = np.empty(L, np.int32)  # 0 wall, 1 floor, 2 free space, 3 volume, 4 empty, 5 side wall
    for l in range(L):
        if l < nA:
            kind[l] = (0, 1, 2, 5)[(l // 64 + l) % 4]
            if kind[l] == 0:
                X[l] = [3.0 + 1e-3 * rng.standard_normal(), rng.uniform(-1.4, 1.4), rng.uniform(0.2, 1.9)]
            elif kind[l] == 1:
                X[l] = [rng.uniform(2.2, 2.9), rng.uniform(-1.0, 1.0), 1e-3 * rng.standard_normal()]
            elif kind[l] == 5:
                X[l] = [rng.uniform(1.9, 2.9), -1.2 + 1e-3 * rng.standard_normal(), rng.uniform(0.2, 1.7)]
            else:
                X[l] = [rng.uniform(1.5, 2.5), rng.uniform(-0.3, 0.3), rng.uniform(1.5, 1.9)]
        elif l < nA + nB:
            kind[l] = 3
            b = blobs[l % len(blobs)]
            X[l] = mean[b] + np.linalg.cholesky(cov[b].reshape(3, 3)) @ rng.standard_normal(3)
        else:
            kind[l] = 4
            X[l] = [2.0, 0.0, 1.0]
    T = synth.look_at_pose(EYE, TARGET)
    pc = X @ synth.quat_to_R(T[:4]).T + T[4:]
    octave = rng.integers(0, 8, L).astype(np.int32)
    sig = 0.5 * 1.2 ** octave
    u = cam.fx * pc[:, 0] / pc[:, 2] + cam.cx + rng.standard_normal(L) * sig
    v = cam.fy * pc[:, 1] / pc[:, 2] + cam.cy + rng.standard_normal(L) * sig
    ur = u - cam.bf / pc[:, 2] + rng.standard_normal(L) * sig * 0.5
    # (a point without an association keeps its stereo observation: the depth of a monocular one would be anybody's guess)
    mono = (rng.uniform(size=L) < 0.15) & (kind != 2)
    ur = np.where(mono, -1.0, np.maximum(ur, 0.0)).astype(np.float32).astype(np.float64)
    octave[kind == 4] = -1
    return dict(pose_init=synth.perturb_pose(T, rng), pose_gt=T, Xw=np.ascontiguousarray(X), obs=np.ascontiguousarray(np.stack([u, v, ur], 1)),
                octave=octave, kind=kind)


def expected_assoc_ok(f, a_gate, wall, floor, blobs, side):
    """the frame is what it was built to be (the oracle's association, not the device's): every kind present, -1 where meant"""
    k = f["kind"][f["octave"] >= 0]
    assert (a_gate[k == 0] == wall).mean() > 0.9 and (a_gate[k == 1] == floor).mean() > 0.9 and (a_gate[k == 5] == side).mean() > 0.9
    assert (a_gate[k == 2] == -1).all() and (k == 2).sum() > 0
    assert np.isin(a_gate[k == 3], list(blobs) + [-1]).all() and np.isin(a_gate[k == 3], blobs).sum() >= 2


def run(torch, ctx, g, cam, prm, frames, prior=None, want_d2=True):
    T = lambda key: torch.from_numpy(np.ascontiguousarray(np.stack([f[key] for f in frames]))).cuda()
    pose, Xw = T("pose_init"), T("Xw")
    if prior is None:
        assoc, d2 = gmmloc_amd.track_frames(ctx, g, cam, prm, pose, Xw, T("obs"), T("octave"), want_d2=want_d2)
    else:
        assoc, d2, _ = gmmloc_amd.track_frames_anchored(ctx, g, cam, prm, pose, Xw, T("obs"), T("octave"),
                                                        prior=torch.from_numpy(np.asarray(prior, np.uint8)).cuda())
    torch.cuda.synchronize()
    return pose.cpu().numpy(), Xw.cpu().numpy(), assoc.cpu().numpy(), d2.cpu().numpy() if d2 is not None else None


def check_against_oracle(oracle, h, cam, frames, res, names, prior=None):
    """the comparison of test_track_frames_matches_oracle, with its tolerances"""
    pose, Xw, assoc, d2 = res
    for i, f in enumerate(frames):
        if prior is None:
            keep, p_ref, pts_ref, a_ref, idx0, d20 = oracle_track(oracle, h, cam, f)
            assert np.array_equal(d2[i][keep], d20)
            expected_assoc_ok(f, np.where(d20 <= 9.0, idx0, -1), *names)
        else:
            keep, p_ref, pts_ref, a_ref, _ = oracle_anchored(oracle, h, cam, f, bool(prior[i]), 0)
        dt, dr = pose_err(pose[i], p_ref)
        assert dt < 1e-6 and dr < 1e-6, (i, dt, dr)
        assert np.array_equal(assoc[i][keep], a_ref), (i, int((assoc[i][keep] != a_ref).sum()))
        err = np.abs(Xw[i][keep] - pts_ref).max(1)
        stereo = f["obs"][keep][:, 2] >= 0
        assert err[stereo].max() < 1e-6 and err.max() < 5e-6, (i, int(np.argmax(err)), err.max())
        assert (assoc[i][f["octave"] < 0] == -1).all()
        assert np.array_equal(Xw[i][f["octave"] < 0], f["Xw"][f["octave"] < 0])


K_SMALL = 24
NAMES_SMALL = (0, K_SMALL - 1, (7, 11, 16), 5)  # (wall, floor, volumes, side wall): component 0 and component K - 1 among the planes


# L = 65: two chunks, G = 1, S = 2, one lane in the last chunk; 256: one wave, all four fields of the packed word; 257: G = 2, slots of
# unequal count; 2000: G = 8, S = 4
@pytest.mark.parametrize("L", [65, 256, 257, 2000])
def test_resident_associations_match_oracle_and_latency_shape(gpu, oracle, opt, L):
    torch, ctx = gpu
    cam, prm = api.Camera(), api.Params()
    mean, cov = build_map(K_SMALL, *NAMES_SMALL)
    frames = [build_frame(mean, cov, cam, L, 100 * L + i, *NAMES_SMALL, empties=(i == 0)) for i in range(2)]
    g = api.GMM(ctx, mean, cov)
    h = oracle.gmm_create(mean, cov)
    res = {}
    for shape in (0, 1):  # the batch shape (resident associations), the latency shape
        opt("ba_shape", shape)
        res[shape] = run(torch, ctx, g, cam, prm, frames)
    for a, b, what in zip(res[0], res[1], ("pose", "points", "assoc", "chi2")):
        assert a.tobytes() == b.tobytes(), (L, what)
    # without the chi2 output the association itself answers -1 above the gate and the set-up has nothing to gate: the same bits
    opt("ba_shape", 0)
    for a, b, what in zip(res[0], run(torch, ctx, g, cam, prm, frames, want_d2=False), ("pose", "points", "assoc")):
        assert a.tobytes() == b.tobytes(), (L, what, "want_d2=False")
    check_against_oracle(oracle, h, cam, frames, res[0], NAMES_SMALL)
    oracle.gmm_destroy(h)


def test_map_of_more_than_65536_components(gpu, oracle, opt):
    """the named components sit above index 65 535; the components that share their low 16 bits are other planes"""
    torch, ctx = gpu
    cam, prm = api.Camera(), api.Params()
    K = 65536 + 512
    names = (65536 + 5, K - 1, (65536 + 100, 300, 65536 + 411), 65535)
    mean, cov = build_map(K, *names)
    frames = [build_frame(mean, cov, cam, 256, 77, *names, empties=True)]
    g = api.GMM(ctx, mean, cov)
    h = oracle.gmm_create(mean, cov)
    opt("ba_shape", 0)
    res = run(torch, ctx, g, cam, prm, frames)
    check_against_oracle(oracle, h, cam, frames, res, names)
    assert (res[2] >= 65536).sum() > 100  # (equal to the oracle's by now: the frame does sit on the components above 65 535)
    oracle.gmm_destroy(h)


def test_anchored_call(gpu, oracle, opt):
    torch, ctx = gpu
    cam, prm = api.Camera(), api.Params()
    mean, cov = build_map(K_SMALL, *NAMES_SMALL)
    frames = [build_frame(mean, cov, cam, 256, 900 + i, *NAMES_SMALL, empties=(i == 0)) for i in range(2)]
    g = api.GMM(ctx, mean, cov)
    h = oracle.gmm_create(mean, cov)
    opt("ba_shape", 0)
    prior = [1, 0]  # (frame 1 rides unanchored in the same call)
    res = run(torch, ctx, g, cam, prm, frames, prior=prior)
    check_against_oracle(oracle, h, cam, frames, res, NAMES_SMALL, prior=prior)
    oracle.gmm_destroy(h)
