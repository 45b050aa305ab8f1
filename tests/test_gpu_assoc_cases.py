"""GPU: every hand-built association case (tests/assoc_cases.py) through the exact cell index, the two all-pairs sweeps, the oracle and
the bit-exact host model (tests/assoc_model.py); the gate.tip, gate.wide, gate.aabb and edge.wide cases through gl_track_frames without d2, the path that never
re-sweeps.  Every map that is meant to use the index is asserted to: index_info()["enabled"], and the `always` count the case declares.

  GL_ASSOC_BRUTE with assoc_index_min = 0   assoc_cell8 {1, 0} (the map is built under it) x assoc_coop {1, 0}; the points are repeated
                                            to 4 096 and more, where the cooperative kernel starts
"""
import numpy as np
import pytest

import gmmloc_amd
from gmmloc_amd import api, synth
from tests import assoc_cases as ac
from tests import assoc_model as am
from tests import optim_cases as oc

pytestmark = pytest.mark.gpu
CAM = oc.camera(oc.CAM5)


def cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def build(gpu, opt, c, mean=None, cov=None, **more):
    """the case's map under the options it declares (they are read when the index is built)"""
    for k, v in dict(c.options, **more).items():
        opt(k, v)
    g = api.GMM(gpu[1], c.mean if mean is None else mean, (c.cov if cov is None else cov).reshape(-1, 9))
    info = g.index_info()
    assert info["enabled"] == c.enabled, (c, info)
    if c.enabled:
        assert info["cell"] == ac.CELL and info["always"] == c.always, (c, info)
    return g, info


def padded(pts, n=4096):
    """the points repeated until there are at least n: from 4 096 points on the cooperative kernel runs"""
    return np.ascontiguousarray(np.tile(pts, (-(-n // len(pts)), 1)))


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


@pytest.mark.parametrize("name", ac.names())
def test_device_arithmetic_is_the_models(gpu, opt, name):
    """Pin the model: F_COV_INV of every component and idx / d2 of ASSOC_EXHAUSTIVE on every case point equal the model's bits."""
    torch, ctx = gpu
    c = ac.CASES[name]
    g, _ = build(gpu, opt, c)
    inv = g.get(api.F_COV_INV)
    want = np.array([am.record(m, cv)[3:] for m, cv in zip(c.mean, c.cov)])
    assert np.array_equal(inv, want, equal_nan=True)
    idx, d2 = g.associate3d(cuda(torch, c.pts), api.ASSOC_EXHAUSTIVE)
    m = c.model()
    assert np.array_equal(idx.cpu().numpy(), m["idx"]) and np.array_equal(d2.cpu().numpy(), m["d2"])


@pytest.mark.parametrize("name", ac.names())
def test_case_through_the_index(gpu, oracle, opt, name):
    """idx and d2 of GL_ASSOC_BRUTE through the index - 8- and 16-byte cells, cooperative gather and a lane per record - equal
    ASSOC_EXHAUSTIVE and ASSOC_SCREENED bit for bit, and all equal the oracle's associate3d, the model and the declared winners."""
    torch, ctx = gpu
    c = ac.CASES[name]
    pts = padded(c.pts)
    assert len(pts) >= 4096 and len(pts) % len(c.pts) == 0
    rep = len(pts) // len(c.pts)
    h = oracle.gmm_create(c.mean, c.cov.reshape(-1, 9))
    try:
        with np.errstate(all="ignore"):
            ref = oracle.associate3d(h, c.pts)
    finally:
        oracle.gmm_destroy(h)
    m = c.model()
    assert np.array_equal(ref[0], m["idx"]) and np.array_equal(ref[1], m["d2"])
    said = c.winner >= 0
    assert np.array_equal(ref[0][said], c.winner[said])
    ref = (np.tile(ref[0], rep), np.tile(ref[1], rep))
    t = cuda(torch, pts)
    opt("assoc_index_min", 0)  # small problems default to the sweep: force the index
    for cell8 in (1, 0):
        g, info = build(gpu, opt, c, assoc_cell8=cell8)
        if c.enabled:
            assert info["bytes"]["packed_cells"] == (8 if cell8 else 16) * int(np.prod(info["dims"])), info
        ex = [x.cpu().numpy() for x in g.associate3d(t, api.ASSOC_EXHAUSTIVE)]
        sc = [x.cpu().numpy() for x in g.associate3d(t, api.ASSOC_SCREENED)]
        assert same(ex, ref), (c, "exhaustive")
        assert same(sc, ref), (c, "screened")
        for coop in (1, 0):
            opt("assoc_coop", coop)
            br = [x.cpu().numpy() for x in g.associate3d(t, api.ASSOC_BRUTE)]
            bad = np.nonzero((br[0] != ref[0]) | (br[1] != ref[1]))[0]
            assert same(br, ref), (c, cell8, coop, len(bad), bad[:8], br[0][bad[:8]], ref[0][bad[:8]], br[1][bad[:8]], ref[1][bad[:8]])
        g.close()


def run_track(gpu, g, datas):
    torch, ctx = gpu
    pose, Xw = cuda(torch, np.stack([d["pose"] for d in datas])), cuda(torch, np.stack([d["Xw"] for d in datas]))
    assoc, d2 = gmmloc_amd.track_frames(ctx, g, CAM, api.Params(), pose, Xw, cuda(torch, np.stack([d["obs"] for d in datas])),
                                        cuda(torch, np.stack([d["oct"] for d in datas])), want_d2=False)
    torch.cuda.synchronize()
    assert d2 is None
    return assoc.cpu().numpy(), pose.cpu().numpy(), Xw.cpu().numpy()


@pytest.mark.parametrize("name", [n for n in ac.names() if ac.CASES[n].track])
def test_case_through_track_frames_without_d2(gpu, oracle, opt, name):
    """gl_track_frames without d2 uses the index whenever it is enabled and never re-sweeps: one frame per scan point (the exactly
    projecting scene of tests/optim_cases.py, point 5 on the scan point).  Association, pose and points by the bytes equal the same
    call with assoc_grid = 0, and the association is the oracle's argmin gated at 9."""
    torch, ctx = gpu
    c = ac.CASES[name]
    picks = ac.track_points(c)
    assert len(picks) >= (3 if name.startswith("edge.") else 8)
    datas = [ac.track_scene(c, n) for n in picks]
    mean, cov = datas[0]["mean"], datas[0]["cov"]
    g, info = build(gpu, opt, c, mean=mean, cov=cov)
    assert info["enabled"]
    with_grid = run_track(gpu, g, datas)
    opt("assoc_grid", 0)
    without = run_track(gpu, g, datas)
    for a, b, what in zip(with_grid, without, ("assoc", "pose", "points")):
        assert a.tobytes() == b.tobytes(), (c, what, np.nonzero(a != b))
    h = oracle.gmm_create(mean, cov.reshape(-1, 9))
    try:
        for d, n, got in zip(datas, picks, with_grid[0]):
            idx, d2 = oracle.associate3d(h, d["Xw"])
            assert np.array_equal(got, np.where(d2 <= 9.0, idx, -1)), (c, n, got, idx, d2)
            assert idx[ac.TRACK_SLOT] == c.model()["idx"][n] and d2[ac.TRACK_SLOT] == c.model()["d2"][n]
    finally:
        oracle.gmm_destroy(h)
    # the picks are on both sides of the gate, so both answers occur
    slot = with_grid[0][:, ac.TRACK_SLOT]
    assert (slot >= 0).any() and (slot < 0).any()


def test_always_unchanged_on_the_reference_maps(gpu, map_v1, map_v2):
    """The admission by the error bound sends no component of the EuRoC maps and of the synthetic bench maps to the global list: their thin
    components are planes (and axis-aligned needles of condition 4e5 at most, bound 2e-4: registered, at a gate of their own).  The
    counts are those of the parent commit."""
    torch, ctx = gpu
    got = {}
    for name, (mean, cov) in (("map_v1", map_v1), ("map_v2", map_v2), ("synth4096_1", synth.synth_gmm(4096, 1)),
                              ("synth65536_5", synth.synth_gmm(65536, 5))):
        g = api.GMM(ctx, mean, cov)
        info = g.index_info()
        assert info["enabled"], name
        got[name] = info["always"]
        g.close()
    print(got)
    assert got == {"map_v1": 0, "map_v2": 0, "synth4096_1": 0, "synth65536_5": 0}  # parent: 0, 0, 0, 0
