"""The batch refine makes each frame's records in its own set-up (gl_ba_fast_impl.hpp: ba1_front; option ba_front, default 1) where
k_ba1_prep made them for the whole launch: the gate, the flag words, the stable three-class partition, the normalised observations,
kept per WORKGROUP and rewritten frame after frame by a persistent one.  Every case runs the same call with ba_front 1 and 0 and wants
pose, points and association equal bit for bit - the path with k_ba1_prep is what the rest of the suite holds to the oracle.  Which
path ran is read off the context's timers: the fused call launches no k_ba1_prep (TIMER_BA_PREP counts 0), every other call at least
one."""
import numpy as np
import pytest

import gmmloc_amd
from gmmloc_amd import synth, api
from tests.context_cases import close_context, new_context
from tests.test_gpu_pose import make_frames
from tests.test_gpu_refine_resident_assoc import NAMES_SMALL, build_frame, build_map, _cov

pytestmark = pytest.mark.gpu

WHAT = ("pose", "points", "assoc")


def call(torch, ctx, g, cam, prm, frames, front, want_d2=False, prior=None, options=()):
    """one gl_track_frames* call on the batch shape; -> (pose, points, assoc, launches of k_ba1_prep)"""
    T = lambda key: torch.from_numpy(np.ascontiguousarray(np.stack([f[key] for f in frames]))).cuda()
    keep = {}
    for name, v in (("ba_shape", 0), ("ba_front", front)) + tuple(options):
        keep.setdefault(name, ctx.get_option(name))
        ctx.set_option(name, v)
    try:
        pose, Xw = T("pose_init"), T("Xw")
        ctx.timing(True)
        ctx.timing_read(api.TIMER_BA_PREP)
        if prior is None:
            assoc, _ = gmmloc_amd.track_frames(ctx, g, cam, prm, pose, Xw, T("obs"), T("octave"), want_d2=want_d2)
        else:
            assoc, _, _ = gmmloc_amd.track_frames_anchored(ctx, g, cam, prm, pose, Xw, T("obs"), T("octave"), want_d2=want_d2,
                                                           prior=torch.from_numpy(np.asarray(prior, np.uint8)).cuda())
        torch.cuda.synchronize()
        nprep = ctx.timing_read(api.TIMER_BA_PREP)[1]
        ctx.timing(False)
    finally:
        for name, v in keep.items():
            ctx.set_option(name, v)
    return pose.cpu().numpy(), Xw.cpu().numpy(), assoc.cpu().numpy(), nprep


def same_bits(a, b, note):
    for x, y, what in zip(a[:3], b[:3], WHAT):
        assert x.tobytes() == y.tobytes(), (note, what, int((x != y).sum()))


def fused_equals_plain(torch, ctx, g, cam, prm, frames, note, options=()):
    fused = call(torch, ctx, g, cam, prm, frames, 1, options=options)
    plain = call(torch, ctx, g, cam, prm, frames, 0, options=options)
    assert fused[3] == 0 and plain[3] >= 1, (note, "k_ba1_prep launches", fused[3], plain[3])
    same_bits(fused, plain, note)
    return fused, plain


# every edge of the canonical order (chunks of 64, G groups, S slots), of the front's rounds (64 G threads) and of the LDS classes
STRIDES = [1, 63, 64, 65, 255, 256, 257, 496, 497, 1000, 1001, 1999, 2000]
_maps = {}


def the_map(ctx, map_v1, name):
    if name not in _maps:
        mean, cov = map_v1 if name == "v1" else synth.synth_gmm(4096, 1)
        _maps[name] = (mean, cov, api.GMM(ctx, mean, cov))
    return _maps[name]


def stride_frames(mean, cov, gt_sync, cam, L, seed):
    frames = make_frames(mean, cov, gt_sync["V1_02_medium"], cam, 3, L, seed, outlier_frac=0.05)
    frames[1]["octave"][::5] = -1  # slots without a map point, scattered: the partition moves them behind the others
    return frames


@pytest.mark.parametrize("mapname", ["v1", "synth"])
@pytest.mark.parametrize("L", STRIDES)
def test_strides(gpu, map_v1, gt_sync, mapname, L):
    torch, ctx = gpu
    cam, prm = api.Camera(), api.Params()
    mean, cov, g = the_map(ctx, map_v1, mapname)
    frames = stride_frames(mean, cov, gt_sync, cam, L, 300 + L)
    fused, _ = fused_equals_plain(torch, ctx, g, cam, prm, frames, (mapname, L))
    assert (fused[2][1][::5] == -1).all()


# ---- a hand-built map, one frame per decision -----------------------------------------------------------------------------------
WALL, FLOOR, BLOBS, SIDE = NAMES_SMALL
K_BASE = 512  # (the few dozen components that matter and patches far behind the camera: a smaller map gets no cell index)
TWIN, NEEDLE, PILE = K_BASE, K_BASE + 1, range(K_BASE + 2, K_BASE + 8)


def hand_map():
    """the map of tests/test_gpu_refine_resident_assoc.py (three planes, three volumes, patches far behind the camera) and: a copy of
    the first volume at a higher index (an exact tie of the two chi2: the lower index wins), a needle of condition 1e10 far away (no
    bound: the association's global list), six small planes of different normals through one spot (a cell of more than three
    candidates; cells at its rim hold fewer)"""
    mean, cov = build_map(K_BASE, *NAMES_SMALL)
    mean = np.concatenate([mean, np.zeros((8, 3))])
    cov = np.concatenate([cov, np.zeros((8, 9))])
    mean[TWIN], cov[TWIN] = mean[BLOBS[0]], cov[BLOBS[0]]
    mean[NEEDLE], cov[NEEDLE] = [-30.0, 0.0, 0.0], _cov([0.0, 0.0, 1.0], [1e-10, 1.0, 1.0]).reshape(9)
    for j, k in enumerate(PILE):
        mean[k] = [2.0, 0.95, 1.5]
        cov[k] = _cov([np.cos(0.5 * j), np.sin(0.5 * j), 0.3 * j - 0.7], [1e-4, 2e-3, 3e-3]).reshape(9)
    return mean, np.ascontiguousarray(cov)


def hand_frames(mean, cov, cam, L):
    rng = np.random.default_rng(L)
    base = lambda seed, empties: build_frame(mean, cov, cam, L, seed, *NAMES_SMALL, empties=empties)
    frames, names = [], []

    def add(name, f):
        names.append(name)
        frames.append(f)

    add("as built: planes and free space, then the volumes, then the empty slots", base(1, True))
    f = base(2, True)  # the same kinds in random slots: volumes and empty slots that the partition has to move
    p = rng.permutation(L)
    for key in ("Xw", "obs", "octave", "kind"):
        f[key] = np.ascontiguousarray(f[key][p])
    add("volumes and empty slots scattered", f)
    f = base(3, False)
    f["octave"][:] = -1
    add("only empty slots", f)
    f = base(4, False)  # every point in free space, far from every component: no association at all
    f["Xw"] = np.ascontiguousarray(np.stack([rng.uniform(1.5, 2.5, L), rng.uniform(-0.3, 0.3, L), rng.uniform(1.6, 1.9, L)], 1))
    add("no association", f)
    f = base(5, False)  # at the gate from both sides: along the wall's normal at 3 sigma (1 +- k 2^-52), k = 0, 1, 2, 4 .. 2^31
    sig = np.sqrt(1e-6)  # (chi2 in (9, 9 (1 + 1e-6)] - resolved by the cell index, dropped by the gate - is among them)
    ks = np.array([0.0] + [2.0 ** e for e in range(32)])
    for i, (k, sgn) in enumerate([(k, s) for k in ks for s in (1.0, -1.0)]):
        if i >= L:
            break
        f["Xw"][i] = [3.0 + 3.0 * sig * (1.0 + sgn * k * 2.0 ** -52), 0.0, 1.2]  # (on the normal through the mean)
    add("at the gate", f)
    f = base(6, False)  # points in the twin volumes (tie), in the pile (long and short lists), outside the map's box on each side
    n = min(L, 48)
    Lc = np.linalg.cholesky(cov[BLOBS[0]].reshape(3, 3))
    for i in range(n):
        if i % 3 == 0:
            f["Xw"][i] = mean[BLOBS[0]] + 0.5 * Lc @ rng.standard_normal(3)
        elif i % 3 == 1:
            f["Xw"][i] = mean[PILE[0]] + rng.uniform(-0.03, 0.03, 3)
    for j, (ax, s) in enumerate([(a, s) for a in range(3) for s in (-1.0, 1.0)]):
        if n + j < L:
            f["Xw"][n + j] = mean[WALL]
            f["Xw"][n + j, ax] += s * 500.0
    add("tie, pile, outside the box", f)
    f = base(7, False)  # a NaN coordinate in a slot without a map point: it must not reach anything
    f["Xw"][L // 2, 1] = np.nan
    f["octave"][L // 2] = -1
    add("NaN coordinate in an empty slot", f)
    return frames, names


@pytest.mark.parametrize("L", [65, 257])
def test_hand_built_decisions(gpu, L):
    torch, ctx = gpu
    cam, prm = api.Camera(), api.Params()
    mean, cov = hand_map()
    g = api.GMM(ctx, mean, cov)
    frames, names = hand_frames(mean, cov, cam, L)
    fused, plain = fused_equals_plain(torch, ctx, g, cam, prm, frames, ("hand-built", L))
    a = plain[2]
    at = names.index
    # the frames are what they were built to be (read from the path with k_ba1_prep)
    assert (a[at("only empty slots")] == -1).all() and (a[at("no association")] == -1).all()
    ngate = min(L, 66)
    gate = a[at("at the gate")][:ngate]
    assert (gate == WALL).any() and (gate == -1).any(), "the gate frame has points on both sides of chi2 = 9"
    mixed = a[at("tie, pile, outside the box")]
    n = min(L, 48)
    assert (mixed[:n:3] == BLOBS[0]).sum() >= n // 6 and not (mixed == TWIN).any(), "equal chi2: the lower index"
    assert np.isin(mixed[1:n:3], list(PILE)).sum() >= 2
    assert (mixed[n:n + 6] == -1).all()
    for name in ("as built: planes and free space, then the volumes, then the empty slots", "volumes and empty slots scattered"):
        fr, ai = frames[at(name)], a[at(name)]
        assert np.isin(ai[fr["kind"] == 3], BLOBS).sum() >= 2 and (ai[fr["kind"] == 4] == -1).all() and (ai[fr["kind"] == 0] == WALL).mean() > 0.8
    assert np.isfinite(plain[0]).all()
    assert (a[at("NaN coordinate in an empty slot")][L // 2] == -1)
    g.close()


# ---- a persistent workgroup rewrites its records frame after frame -----------------------------------------------------------------
@pytest.mark.parametrize("persist", [1, 0])
def test_records_reused_by_persistent_workgroups(gpu, map_v1, gt_sync, persist):
    """L = 64 is the class of four frames per CU: with 4 CUs + 3 frames every workgroup of the persistent launch takes a second frame.
    Frames alternate full / all empty / half empty: a record left over from the previous frame would show."""
    torch, ctx = gpu
    cam, prm = api.Camera(), api.Params()
    mean, cov, g = the_map(ctx, map_v1, "v1")
    B = 4 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    kinds = make_frames(mean, cov, gt_sync["V1_02_medium"], cam, 6, 64, 64064, outlier_frac=0.05)
    for i, f in enumerate(kinds):
        if i % 3 == 1:
            f["octave"][:] = -1
        elif i % 3 == 2:
            f["octave"][(i // 3)::2] = -1
    frames = [kinds[i % 6] for i in range(B)]
    fused, _ = fused_equals_plain(torch, ctx, g, cam, prm, frames, ("reuse", persist), options=(("ba_persist", persist),))
    for i in range(6, B):  # (equal inputs, equal outputs - whichever workgroup took the frame, whatever it held before)
        for k in range(3):
            assert fused[k][i].tobytes() == fused[k][i % 6].tobytes(), (i, WHAT[k])


def test_poisoned_context(gpu, map_v1, gt_sync):
    """the first stride case on a new context whose scratch blocks are filled with 0xFF / 0x00 as they are allocated"""
    torch, ctx = gpu
    cam, prm = api.Camera(), api.Params()
    mean, cov, g = the_map(ctx, map_v1, "v1")
    for L in (STRIDES[0], 257):
        frames = stride_frames(mean, cov, gt_sync, cam, L, 300 + L)
        ref = call(torch, ctx, g, cam, prm, frames, 0)
        for fill in (0xFF, 0x00):
            c2 = new_context()
            try:
                c2.set_option("test_scratch_fill", fill)
                g2 = api.GMM(c2, mean, cov)
                got = call(torch, c2, g2, cam, prm, frames, 1)
                assert got[3] == 0
                same_bits(got, ref, ("poisoned", L, fill))
                c2.synchronize()
                g2.close()
            finally:
                close_context(c2)


def test_wide_instances(gpu):
    """a map of more than 65 536 components takes the instances that read the association per pass (bafd*w): they read the front's"""
    torch, ctx = gpu
    cam, prm = api.Camera(), api.Params()
    K = 65536 + 512
    names = (65536 + 5, K - 1, (65536 + 100, 300, 65536 + 411), 65535)
    mean, cov = build_map(K, *names)
    g = api.GMM(ctx, mean, cov)
    for L in (256, 1000, 2000):
        frames = [build_frame(mean, cov, cam, L, 77 + L + i, *names, empties=(i == 0)) for i in range(2)]
        fused, _ = fused_equals_plain(torch, ctx, g, cam, prm, frames, ("wide", L))
        assert (fused[2] >= 65536).sum() > L // 3
    g.close()


def test_fall_backs(gpu, map_v1, gt_sync):
    """want_d2, assoc_grid = 0, the anchored call and the latency shape take the path with k_ba1_prep, with unchanged results, and
    give the association of the fused call"""
    torch, ctx = gpu
    cam, prm = api.Camera(), api.Params()
    mean, cov, g = the_map(ctx, map_v1, "v1")
    frames = stride_frames(mean, cov, gt_sync, cam, 257, 557)
    fused, _ = fused_equals_plain(torch, ctx, g, cam, prm, frames, "fall-backs, fused")
    for note, kw in (("want_d2", dict(want_d2=True)), ("assoc_grid = 0", dict(options=(("assoc_grid", 0),))),
                     ("anchored", dict(prior=[0, 0, 0])), ("latency shape", dict(options=(("ba_shape", 1),)))):
        on, off = call(torch, ctx, g, cam, prm, frames, 1, **kw), call(torch, ctx, g, cam, prm, frames, 0, **kw)
        assert on[3] >= 1 and off[3] >= 1, (note, "k_ba1_prep launches", on[3], off[3])
        same_bits(on, off, note)
        assert np.array_equal(on[2], fused[2]), note
        if note != "anchored":
            same_bits(on, fused, note)
