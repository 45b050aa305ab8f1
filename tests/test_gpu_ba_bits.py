"""The rules of the local BA may be restated, never changed: gl_joint_optimization must return the BITS recorded in
tests/golden/ba_bits_parent.json (sha256 of poses, points, dropped, erase[:nobs] and iters, taken on an MI355X from the commit
before the rules of jointOptimization were stated once for both launch shapes), in the two shapes whose bits do not depend on
what else runs on the device: the persistent kernel with one workgroup per window (bagen_mode 1, bagen_nb 1) and the pipelined
kernels (bagen_mode 2).  One small window per class of the reduced-system solve and its edges (6P <= 32 / 48 / 80 / 128 and
the scalar-pivot path), one with ba_first_as_prior = 0, the stop word set on entry and as a budget of 3 / 5 / 7 outer iterations,
and one batch of three windows of which one has every fourth association -1 and one has none.
tools/record_ba_bits.py writes the file; a case without a recorded hash fails."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from gmmloc_amd import api
from tests.test_gpu_ba import make_ba_problem

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_bits_parent.json")
SHAPES = {"persistent1": (1, 1), "pipelined": (2, 0)}  # name -> (bagen_mode, bagen_nb)
SOLVE = [(1, 0, 120, False), (3, 1, 200, True), (5, 3, 300, True), (6, 2, 500, True), (9, 2, 600, True), (14, 2, 700, True),
         (21, 2, 700, True), (22, 2, 700, True)]


def all_cases():
    """case id -> dict(P, F, L, prior, seeds, first_as_prior, stop, thin: window whose every fourth association is -1,
    none: window without associations)"""
    base = dict(first_as_prior=1, stop=None, thin=-1, none=-1)
    cases = {}
    for P, F, L, prior in SOLVE:
        cases["solve-P%d-F%d-L%d" % (P, F, L)] = dict(base, P=P, F=F, L=L, prior=prior, seeds=(100 + P,))
    cases["fixed-first-P3-F1-L150"] = dict(base, P=3, F=1, L=150, prior=True, seeds=(5,), first_as_prior=0)
    for stop in (1, -3, -5, -7):
        cases["stop%+d-P3-F2-L200" % stop] = dict(base, P=3, F=2, L=200, prior=True, seeds=(293,), stop=stop)
    cases["batch3-P5-F3-L300"] = dict(base, P=5, F=3, L=300, prior=True, seeds=(50, 51, 52), thin=1, none=2)
    return cases


@functools.lru_cache(maxsize=None)
def _problems(cid):
    d = np.load(os.path.join(os.path.dirname(GOLDEN), "map_v1.npz"))
    gt = np.load(os.path.join(os.path.dirname(GOLDEN), "gt_sync.npz"))["V1_01_easy"]
    c = all_cases()[cid]
    return [make_ba_problem(d["mean"], d["cov"], gt, api.Camera(), c["P"], c["F"], c["L"], s, c["prior"]) for s in c["seeds"]]


def run_case(torch, ctx, g, cid, shape):
    """[poses, points, dropped, erase[:nobs], iters] of every window of case `cid` at launch shape `shape`, in that order."""
    c = all_cases()[cid]
    probs = _problems(cid)
    cam, prm = api.Camera(), api.Params(ba_first_as_prior=c["first_as_prior"])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    NOBS = max(len(p["obs_pose"]) for p in probs)

    def stack(key):
        out = np.zeros((len(probs), NOBS) + probs[0][key].shape[1:], probs[0][key].dtype)
        for b, p in enumerate(probs):
            out[b, :len(p[key])] = p[key]
        return T(out)

    points = T(np.stack([p["points"] for p in probs]))
    idx, d2 = g.associate3d(points.reshape(-1, 3))
    assoc = torch.where(d2 <= 9.0, idx, torch.full_like(idx, -1)).reshape(len(probs), c["L"]).contiguous()
    if c["thin"] >= 0:
        assoc[c["thin"], ::4] = -1
    if c["none"] >= 0:
        assoc[c["none"], :] = -1
    poses = T(np.stack([p["poses"] for p in probs]))
    stop = None if c["stop"] is None else torch.tensor([c["stop"]], dtype=torch.int32).cuda()
    mode, nb = SHAPES[shape]
    old = {k: ctx.get_option(k) for k in ("bagen_mode", "bagen_nb")}
    ctx.set_option("bagen_mode", mode)
    ctx.set_option("bagen_nb", nb)
    try:
        dropped, erase, iters = api.joint_optimization(ctx, g, cam, prm, c["P"], c["F"], poses, T(np.stack([p["prior"] for p in probs])),
                                                       points, assoc, T(np.stack([p["obs_ptr"] for p in probs])), stack("obs_pose"),
                                                       stack("obs_uvr"), stack("obs_oct"), stop_flag=stop)
        torch.cuda.synchronize()
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)
    out = []
    for b, p in enumerate(probs):
        out += [poses[b].cpu().numpy(), points[b].cpu().numpy(), dropped[b].cpu().numpy(), erase[b].cpu().numpy()[:len(p["obs_pose"])],
                iters[b:b + 1].cpu().numpy()]
    return out


def digest(res):
    h = hashlib.sha256()
    for a in res:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def case_id(cid, shape):
    return "%s-%s" % (cid, shape)


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as fh:
        return json.load(fh)["sha256"]


@pytest.fixture(scope="module")
def gmm(gpu, map_v1):
    return api.GMM(gpu[1], *map_v1)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("cid", list(all_cases()))
def test_ba_bits_match_parent(gpu, gmm, recorded, cid, shape):
    torch, ctx = gpu
    res = run_case(torch, ctx, gmm, cid, shape)
    c = all_cases()[cid]
    if c["stop"] == 1:  # set on entry: nothing is written
        p = _problems(cid)[0]
        assert np.array_equal(res[0], p["poses"]) and np.array_equal(res[1], p["points"]) and not res[2].any() and not res[3].any()
        assert int(res[4][0]) == 0
    key = case_id(cid, shape)
    got = digest(res)
    print(key, got)
    assert key in recorded, "no hash recorded for %s" % key
    assert got == recorded[key], key
