"""The refine's reductions and hand-over may be rearranged, never re-ordered: gl_track_frames / gl_track_frames_anchored must
return the BITS recorded in tests/golden/refine_bits_parent.json (sha256 of pose, points and associations, taken on an MI355X
from the commit before the reductions of k_ba1_fast were slimmed), and the batch shape (DENSE) and the latency shape (SPREAD)
must agree bit for bit.  The sizes are the smallest at which a reduction can go wrong: a partly filled chunk, one full chunk,
one group of three chunks, a short second group, the first and the full size of every wave class, a last chunk of one point.
Every batch carries its B frames (5 % outliers, 10 % of the octaves -1) and one more frame without any map point.
tools/record_refine_bits.py writes the file; a case without a recorded hash fails."""
import hashlib
import json
import os

import numpy as np
import pytest

import gmmloc_amd
from gmmloc_amd import api
from tests.test_gpu_pose import make_frames

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_bits_parent.json")
CASES = [(37, 2), (64, 1), (130, 3), (257, 2), (496, 2), (513, 2), (1000, 2), (1025, 2), (1985, 1), (2000, 2)]
ANCHORED = [(1000, 2), (2000, 2)]
WHAT = ("pose", "points", "assoc")


def build_frames(map_v1, gt_sync, M, B):
    mean, cov = map_v1
    frames = make_frames(mean, cov, gt_sync["V1_02_medium"], api.Camera(), B + 1, M, 1000 + M, outlier_frac=0.05)
    rng = np.random.default_rng(77 + M)
    for f in frames[:B]:
        f["octave"][rng.uniform(size=M) < 0.1] = -1
    frames[B]["octave"][:] = -1
    return frames


def run_case(torch, ctx, g, frames, shape, anchored):
    """(pose, points, assoc) of one call at launch shape `shape` (0: DENSE, 1: SPREAD)."""
    cam, prm = api.Camera(), api.Params()
    T = lambda k: torch.from_numpy(np.stack([f[k] for f in frames])).cuda()
    pose, Xw = T("pose_init"), T("Xw")
    old = ctx.get_option("ba_shape")
    ctx.set_option("ba_shape", shape)
    try:
        if anchored:
            prior = torch.ones(len(frames), dtype=torch.uint8).cuda()
            assoc = gmmloc_amd.track_frames_anchored(ctx, g, cam, prm, pose, Xw, T("obs"), T("octave"), prior=prior)[0]
        else:
            assoc = gmmloc_amd.track_frames(ctx, g, cam, prm, pose, Xw, T("obs"), T("octave"))[0]
        torch.cuda.synchronize()
    finally:
        ctx.set_option("ba_shape", old)
    return pose.cpu().numpy(), Xw.cpu().numpy(), assoc.cpu().numpy()


def digest(res):
    h = hashlib.sha256()
    for a in res:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def case_id(M, B, shape, anchored):
    return "%s-M%d-B%d-shape%d" % ("anchored" if anchored else "plain", M, B, shape)


def all_case_params():
    return [(M, B, False) for M, B in CASES] + [(M, B, True) for M, B in ANCHORED]


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as fh:
        return json.load(fh)["sha256"]


@pytest.mark.parametrize("M,B,anchored", all_case_params())
def test_refine_bits_match_parent(gpu, map_v1, gt_sync, recorded, M, B, anchored):
    torch, ctx = gpu
    mean, cov = map_v1
    g = api.GMM(ctx, mean, cov)
    frames = build_frames(map_v1, gt_sync, M, B)
    res = {shape: run_case(torch, ctx, g, frames, shape, anchored) for shape in (0, 1)}
    # (a) DENSE == SPREAD
    for a, b, what in zip(res[0], res[1], WHAT):
        assert np.array_equal(a, b, equal_nan=True), (M, B, anchored, what)
    # (b) the parent's bits
    for shape in (0, 1):
        cid = case_id(M, B, shape, anchored)
        got = digest(res[shape])
        print(cid, got)
        assert cid in recorded, "no hash recorded for %s" % cid
        assert got == recorded[cid], cid
