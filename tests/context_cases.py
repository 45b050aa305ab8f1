"""One table of calls for tests/test_gpu_context_state.py: every public entry point that carves a region out of one of the context's
scratch blocks (gl_internal.hpp: SCRATCH_MAIN ... SCRATCH_MAPEDIT) or reads other state a context carries from call to call (the staging
buffers, pipe_hint, the lds_limit / occupancy caches, the event pool, the statistics buffers) - and, to keep the table the whole public
surface, the few that use none.  DESIGN.md ("What a context carries from call to call") has the regions of every entry point and the
kernel that initialises each.

A case is a pair of callables, small(torch, ctx) and large(torch, ctx): each makes ONE call (or the fixed short sequence that is the
entry point's use: search2d -> check_map_association, searchForTriangulation -> gather) on inputs from pinned seeds and returns a dict
of numpy arrays with every output of the call, the inputs it updates in place included.  The inputs are made once per process and
uploaded afresh for every call, so every call of `small` gets the same bytes.  The GMM is map_v1, built once per context (gmm_of).

Shapes: `small` sits off every wave (64) and block (256) multiple; `large` is at least twice `small` in every dimension and crosses the
next launch-shape or LDS-class threshold its entry point has (named in the table below), so that the regions of `small` land in the
middle of what `large` left behind.  Each callable asserts that its call was not trivial (matches found, points kept, key-frames
culled ...).

Test infrastructure; nothing in the product imports it."""
import contextlib
import functools
import os

import numpy as np

import gmmloc_amd
from gmmloc_amd import api, synth
from tests import ba_window_ref as BR
from tests import ba_window_scenes as BS
from tests import chain_glue as G
from tests import configs
from tests import local_map_ref as LR
from tests import local_map_scenes as LS
from tests import map_edit_ref as ER
from tests import map_edit_scenes as ES
from tests.chain_glue import TH_LOCAL, TH_MM
from tests.gpu_helpers import T, to_dev

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------- shared inputs
@functools.lru_cache(maxsize=None)
def map_v1():
    d = np.load(os.path.join(GOLDEN, "map_v1.npz"))
    return d["mean"], d["cov"]


@functools.lru_cache(maxsize=None)
def gt_sync():
    return dict(np.load(os.path.join(GOLDEN, "gt_sync.npz")))


def gmm_of(ctx):
    """the context's GMM of map_v1, built at its first use"""
    if getattr(ctx, "_case_gmm", None) is None:
        ctx._case_gmm = api.GMM(ctx, *map_v1())
    return ctx._case_gmm


def new_context():
    return gmmloc_amd.Context(0)


def close_context(ctx):
    g = getattr(ctx, "_case_gmm", None)
    if g is not None:
        ctx.synchronize()
        g.close()
        ctx._case_gmm = None
    ctx.close()


@contextlib.contextmanager
def options(ctx, **kw):
    """the options of one call, put back afterwards (nothing else is touched: the legs set test_scratch_fill themselves)"""
    saved = {k: ctx.get_option(k) for k in kw}
    for k, v in kw.items():
        ctx.set_option(k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


def H(torch, d):
    """dict / sequence of tensors -> dict of numpy arrays, after the work is complete"""
    torch.cuda.synchronize()
    if not isinstance(d, dict):
        d = {"out%d" % i: v for i, v in enumerate(d)}
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in d.items() if v is not None}


CAM, PRM = api.Camera, api.Params


class Case:
    def __init__(self, name, entries, small, large, check=None, opts=None):
        """entries: the api wrappers the case calls; check(oracle, out): the cold result of `small` against the oracle (the composites
        and track_frames); opts: options both callables run under"""
        self.name, self.entries, self.check, self.opts = name, tuple(entries), check, dict(opts or {})
        self.small, self.large = self._wrap(small), self._wrap(large)

    def _wrap(self, fn):
        def run(torch, ctx):
            with options(ctx, **self.opts):
                return fn(torch, ctx)
        return run

    def __repr__(self):
        return self.name


CASES = []


def case(name, entries, sizes, check=None, opts=None):
    """register fn(torch, ctx, *size) under the two sizes"""
    def deco(fn):
        small, large = sizes
        CASES.append(Case(name, entries, lambda t, c: fn(t, c, *small), lambda t, c: fn(t, c, *large), check, opts))
        return fn
    return deco


# ---------------------------------------------------------------------------------------------------------------- association
@functools.lru_cache(maxsize=None)
def _points(N):
    return synth.synth_points(*map_v1(), N, 40 + N)


def _associate(mode):
    def run(torch, ctx, N):
        idx, d2 = gmm_of(ctx).associate3d(T(torch, _points(N)), mode)
        out = H(torch, dict(idx=idx, d2=d2))
        assert (out["idx"] >= 0).all() and np.isfinite(out["d2"]).all() and len(set(out["idx"].tolist())) > N // 16
        assert (out["d2"] > 9.0).any() and (out["d2"] <= 9.0).any()  # points the cell index resolves and points it leaves to the sweep
        return out
    return run


# (5 000 points: the cooperative gather of the cell index starts at 4 096; K splits and merge of the sweep at every size)
case("associate3d_brute_index", ["associate3d"], ((257,), (5000,)), opts=dict(assoc_index_min=0))(_associate(api.ASSOC_BRUTE))
case("associate3d_exhaustive", ["associate3d"], ((257,), (5000,)))(_associate(api.ASSOC_EXHAUSTIVE))


@case("associate3d_screened", ["associate3d"], ((257,), (5000,)), opts=dict(assoc_screen32=1))
def _associate_screened(torch, ctx, N):
    ctx.counter_read(api.COUNTER_ASSOC_SCREEN_VERIFIED)
    out = _associate(api.ASSOC_EXHAUSTIVE)(torch, ctx, N)
    assert ctx.counter_read(api.COUNTER_ASSOC_SCREEN_VERIFIED) >= N  # the screen ran (its own block) and sent pairs to the fp64 verify
    return out


@case("knn3d_query_point", ["knn3d", "queryPoint"], ((300,), (9300,)))  # a wave per query up to 16 x CUs points, a thread per query above
def _knn(torch, ctx, N):
    g, pts = gmm_of(ctx), T(torch, _points(N))
    idx, dist = g.knn3d(pts, 5)
    q = g.queryPoint(pts)
    out = H(torch, dict(idx=idx, dist=dist, query=q))
    assert np.array_equal(out["idx"][:, 0], out["query"]) and (np.diff(out["dist"], axis=1) >= 0).all() and (out["idx"] >= 0).all()
    return out


@case("search2d", ["search2d"], ((2, 333), (5, 700)))
def _search2d(torch, ctx, B, N):
    cam, gt = CAM(), gt_sync()["V1_01_easy"]
    poses = np.stack([synth.gt_row_to_Tcw(gt[(7 + i * 131) % gt.shape[0]]) for i in range(B)])
    rng = np.random.default_rng(3 + N)
    uv = np.stack([rng.uniform(0, cam.width, (B, N)), rng.uniform(0, cam.height, (B, N))], 2)
    cand, ncand, vids, nview = gmm_of(ctx).search2d(cam, T(torch, poses), T(torch, uv), None, k=5, view_cap=4096)
    out = H(torch, dict(cand=cand, ncand=ncand, vids=vids, nview=nview))
    assert out["nview"].sum() > 50 * B and (out["ncand"] > 0).mean() > 0.5
    return out


# ---------------------------------------------------------------------------------------------------------------- points
@functools.lru_cache(maxsize=None)
def _point_inputs(N):
    import numpy_ref as nr  # (tests/configs.py has put oracle/ on the path)
    from tests.test_oracle_configs import point_inputs
    mean, cov = map_v1()
    seq = gt_sync()["V1_01_easy"]
    world = dict(mean=mean, cov=cov, comps=nr.build_components(mean, cov), seq=seq, poses=np.stack([synth.gt_row_to_Tcw(seq[i]) for i in (50, 900, 2100)]))
    return point_inputs(world, configs.DEFAULT, N=N)


@case("optimize_point", ["optimize_point"], ((130,), (600,)))
def _optimize_point(torch, ctx, N):
    d = _point_inputs(N)
    f = d["f"]
    res = api.optimize_point(ctx, gmm_of(ctx), CAM(), PRM(), T(torch, d["X0"]), T(torch, f["obs"]), T(torch, f["octave"]), T(torch, np.tile(d["pose"], (N, 1))),
                             T(torch, d["comp"]), T(torch, d["pz"]))
    out = H(torch, dict(zip(("res", "chi2_proj", "chi2_str", "est"), res)))
    assert 0 < out["res"].sum() < N
    return out


@case("check_map_association", ["search2d", "check_map_association"], ((130,), (600,)))
def _check_map_association(torch, ctx, N):
    d = _point_inputs(N)
    f, g, cam = d["f"], gmm_of(ctx), CAM()
    octv = f["octave"].copy()
    octv[::9] = -1
    pose = T(torch, d["pose"][None])
    cand, ncand, _, _ = g.search2d(cam, pose, T(torch, f["obs"][None, :, :2]), None, k=5)
    pts = T(torch, d["X0"][None])
    comp = api.check_map_association(ctx, g, cam, PRM(), pose, pts, T(torch, f["obs"][None]), T(torch, octv[None]), cand, ncand)
    out = H(torch, dict(cand=cand, ncand=ncand, comp=comp, pts=pts))
    assert (out["comp"] >= 0).sum() > N // 12 and (out["comp"] < 0).sum() > N // 12
    return out


@case("optimize_triangulation", ["optimize_triangulation"], ((130,), (600,)))
def _optimize_triangulation(torch, ctx, N):
    d = _point_inputs(N)
    f = d["f"]
    n1, n2 = (d["cands"] >= 0).sum(1).astype(np.int32), (d["cands2"] >= 0).sum(1).astype(np.int32)
    oct2 = np.random.default_rng(4).integers(0, 8, N).astype(np.int32)
    x = T(torch, d["X0"])
    comp = api.optimize_triangulation(ctx, gmm_of(ctx), CAM(), PRM(), x, T(torch, np.tile(d["pose"], (N, 1))), T(torch, d["uvr1"]), T(torch, f["octave"]),
                                      T(torch, np.tile(d["pose2"], (N, 1))), T(torch, d["uvr2"]), T(torch, oct2), T(torch, d["cands"]), T(torch, n1),
                                      T(torch, d["cands2"]), T(torch, n2))
    out = H(torch, dict(comp=comp, x3d=x))
    assert N // 20 < (out["comp"] >= 0).sum() < N
    return out


@functools.lru_cache(maxsize=None)
def _tri_matches(N):
    gt = gt_sync()["V1_01_easy"]
    return synth.synth_tri_matches(*map_v1(), synth.gt_row_to_Tcw(gt[900]), synth.gt_row_to_Tcw(gt[915]), CAM(), N, 5)


TRI_KEYS = ("pose1", "uvr1", "depth1", "oct1", "pose2", "uvr2", "depth2", "oct2", "cand1", "n1", "cand2", "n2")


@case("create_map_points", ["create_map_points"], ((130,), (600,)))
def _create_map_points(torch, ctx, N):
    m = _tri_matches(N)
    x, t, c = api.create_map_points(ctx, gmm_of(ctx), CAM(), PRM(), *[T(torch, m[k]) for k in TRI_KEYS])
    out = H(torch, dict(x3d=x, type=t, comp=c))
    assert (out["type"] > 0).sum() > N // 12 and (out["type"] == 0).sum() > 0
    return out


# ---------------------------------------------------------------------------------------------------------------- poses and frames
@functools.lru_cache(maxsize=None)
def _frames(B, M, seed=300):
    from tests.test_gpu_pose import make_frames
    fr = make_frames(*map_v1(), gt_sync()["V1_03_difficult"], CAM(), B, M, seed + M, outlier_frac=0.06)
    fr[1]["octave"][::2] = -1  # a sparse frame: its edges fit a compacted problem where the others' do not
    fr[2]["octave"][::7] = -1
    return fr


def _pose(torch, ctx, B, M):
    from tests.test_gpu_pose import run_gpu
    frames = _frames(B, M)
    pose, outl, nin = run_gpu((torch, ctx), CAM(), PRM(), frames)
    assert (nin > 10).all() and outl.any() and np.abs(pose - np.stack([f["pose_init"] for f in frames])).max() > 1e-4
    return dict(pose=pose, outlier=outl, ninlier=nin)


# (1 200 slots: compacted to 1 024 by default - compaction is on from 1 025 slots)
case("optimize_current_pose", ["optimize_current_pose"], ((3, 300), (5, 1200)))(_pose)
# every problem of more than 256 slots compacted to 256: the full frames overflow into their full-stride problem, the sparse one fits
case("optimize_current_pose_overflow", ["optimize_current_pose"], ((3, 300), (5, 1200)), opts=dict(pose_compact=1, pose_compact_cap=256))(_pose)


def _track(torch, ctx, B, M):
    from tests.test_gpu_track import _run_track
    pose, Xw, assoc, d2 = _run_track(torch, ctx, gmm_of(ctx), CAM(), PRM(), _frames(B, M))
    assert (assoc >= 0).mean() > 0.3 and (assoc < 0).any()
    return dict(pose=pose, Xw=Xw, assoc=assoc, d2=d2)


def _check_track(oracle, out, B=3, M=300):
    """the assertions of tests/test_gpu_track.py::test_track_frames_matches_oracle"""
    from tests.test_gpu_pose import pose_err
    from tests.test_gpu_track import oracle_track
    h = oracle.gmm_create(*map_v1())
    for i, f in enumerate(_frames(B, M)):
        keep, p_ref, pts_ref, a_ref, idx0, d20 = oracle_track(oracle, h, CAM(), f)
        assert np.array_equal(out["d2"][i][keep], d20), i
        dt, dr = pose_err(out["pose"][i], p_ref)
        assert dt < 1e-6 and dr < 1e-6, (i, dt, dr)
        assert np.array_equal(out["assoc"][i][keep], a_ref), (i, int((out["assoc"][i][keep] != a_ref).sum()))
        err = np.abs(out["Xw"][i][keep] - pts_ref).max(1)
        assert err[f["obs"][keep][:, 2] >= 0].max() < 1e-6 and err.max() < 5e-6, (i, err.max())
        assert (out["assoc"][i][f["octave"] < 0] == -1).all()
    oracle.gmm_destroy(h)


# (300 -> 1 001 points: across the 496- and 1 000-point LDS classes of the on-chip refine; both launch shapes)
case("track_frames_batch_shape", ["track_frames"], ((3, 300), (5, 1001)), check=_check_track, opts=dict(ba_shape=0))(_track)
case("track_frames_latency_shape", ["track_frames"], ((3, 300), (5, 1001)), check=_check_track, opts=dict(ba_shape=1))(_track)
case("track_frames_general_kernel", ["track_frames"], ((3, 300), (5, 1001)), check=_check_track, opts=dict(ba_slow=1))(_track)


@functools.lru_cache(maxsize=None)
def _fixed_frames(B, M):
    from tests.test_gpu_anchor import add_fixed
    return [add_fixed(dict(f), CAM(), 2, 900 + i) for i, f in enumerate(_frames(B, M))]


def _anchored(fixed):
    def run(torch, ctx, B, M):
        from tests.test_gpu_anchor import dev
        frames = _fixed_frames(B, M)
        pose, Xw = dev(torch, frames, "pose_init"), dev(torch, frames, "Xw")
        prior = T(torch, (np.arange(B) % 2 == 0).astype(np.uint8))
        kw = dict(fixed_pose=dev(torch, frames, "fixed_pose"), fixed_obs=dev(torch, frames, "fixed_obs"), fixed_oct=dev(torch, frames, "fixed_oct"),
                  want_erase=True) if fixed else {}
        assoc, d2, erase = gmmloc_amd.track_frames_anchored(ctx, gmm_of(ctx), CAM(), PRM(), pose, Xw, dev(torch, frames, "obs"), dev(torch, frames, "octave"),
                                                            prior=prior, **kw)
        out = H(torch, dict(pose=pose, Xw=Xw, assoc=assoc, d2=d2, erase=erase))
        assert (out["assoc"] >= 0).mean() > 0.3 and (not fixed or out["erase"].sum() > 0)
        return out
    return run


case("track_frames_anchored_prior", ["track_frames_anchored"], ((3, 300), (5, 1001)), opts=dict(ba_shape=1))(_anchored(False))
case("track_frames_anchored_fixed", ["track_frames_anchored"], ((3, 300), (5, 1001)))(_anchored(True))
# the same through k_track_pack -> k_ba_gen -> k_track_unpack: the packed problems and the BA's flags live in the scratch block
case("track_frames_anchored_packed", ["track_frames_anchored"], ((3, 300), (5, 1001)), opts=dict(ba_fixed_pack=1))(_anchored(True))


@case("host_track_frame", ["HostFramePath.track_frame"], ((300,), (1200,)))  # the staging buffers grow
def _host_frame(torch, ctx, M):
    f = _frames(3, M)[0]
    path = api.HostFramePath(ctx, gmm_of(ctx), CAM(), PRM())
    out = {}
    for anchored in (False, True):
        pose, Xw = f["pose_init"].copy(), f["Xw"].copy()
        assoc = path.track_frame(pose, Xw, f["obs"], f["octave"], anchored=anchored)
        out.update({"pose%d" % anchored: pose, "Xw%d" % anchored: Xw, "assoc%d" % anchored: assoc})
    assert (out["assoc0"] >= 0).mean() > 0.3 and not np.array_equal(out["pose0"], out["pose1"])
    return out


# ---------------------------------------------------------------------------------------------------------------- the local BA
@functools.lru_cache(maxsize=None)
def _ba_problem(P, F, L, seed):
    from tests.test_gpu_ba import make_ba_problem
    mean, cov = map_v1()
    p = make_ba_problem(mean, cov, gt_sync()["V1_01_easy"], CAM(), P, F, L, seed, True)
    # the association a host would hold: the nearest component by Mahalanobis distance, gated at 9 (an INPUT of the call)
    d = p["points"][:, None, :] - mean[None]
    d2 = np.einsum("nki,kij,nkj->nk", d, np.linalg.inv(cov.reshape(-1, 3, 3)), d)
    k = d2.argmin(1)
    return p, np.where(d2[np.arange(L), k] <= 9.0, k, -1).astype(np.int32)


def _ba(torch, ctx, B, P, F, L, seed, pipelined):
    from tests.test_gpu_ba import run_gpu
    p, a = _ba_problem(P, F, L, seed)
    assert ctx.get_option("bagen_mode") != 0 or (len(p["obs_pose"]) >= 3000) == pipelined, len(p["obs_pose"])
    poses, points, dropped, erase, iters = run_gpu((torch, ctx), gmm_of(ctx), CAM(), PRM(), [p] * B, [a] * B)
    assert (iters > 0).all() and erase.any() and not np.array_equal(poses[0, :P], p["poses"][:P])
    assert all(np.array_equal(x[0], x[b]) for x in (poses, points, dropped, erase, iters) for b in range(B))  # (copies: the same bits)
    return dict(poses=poses, points=points, dropped=dropped, erase=erase, iters=iters)


def _check_ba(P, F, L, seed):
    def check(oracle, out):
        from tests.test_gpu_ba import check as ba_check
        p, a = _ba_problem(P, F, L, seed)
        h = oracle.gmm_create(*map_v1())
        ba_check([p], [a], [out[k] for k in ("poses", "points", "dropped", "erase", "iters")], oracle, h, CAM())
        oracle.gmm_destroy(h)
    return check


# persistent cooperative kernel below 3 000 observations, the pipelined shape from there on
case("joint_optimization", ["joint_optimization"], ((1, 4, 2, 300, 61, False), (1, 8, 4, 1500, 62, True)), check=_check_ba(4, 2, 300, 61))(_ba)
# two pipelined calls next to each other in the table, a window of many Levenberg cycles and one of few: in table order the many-cycle
# window's pipe_hint is what the few-cycle window starts from, in reverse order the other way round.  `large` of the second: 16 copies,
# which the pipelined shape splits over two lanes (streams)
case("joint_optimization_pipelined_many", ["joint_optimization"], ((1, 8, 4, 600, 63, True), (2, 12, 4, 1000, 64, True)), check=_check_ba(8, 4, 600, 63))(_ba)
case("joint_optimization_pipelined_few", ["joint_optimization"], ((1, 2, 1, 150, 65, False), (16, 8, 4, 600, 63, True)), check=_check_ba(2, 1, 150, 65),
     opts=dict(bagen_mode=2))(_ba)


# ---------------------------------------------------------------------------------------------------------------- the matchers
@case("search_by_projection", ["search_by_projection"], ((2, 300, 200), (4, 700, 900)))
def _sbp(torch, ctx, B, NF, NP):
    from tests.test_gpu_match import run_gpu
    m, n = run_gpu(torch, ctx, [synth.synth_match_frame(NF, NP, 1000 * NF + 7 * b, dup_frac=0.3, float_uv=b % 2 == 0) for b in range(B)], 3.0)
    assert n.sum() > 20 * B
    return dict(match=m, nmatches=n)


@case("search_by_projection_frame", ["search_by_projection_frame"], ((2, 300, 200), (4, 700, 900)))
def _sbpf(torch, ctx, B, NF, NL):
    from tests.test_gpu_match import CamF, run_gpu_frame
    m, n = run_gpu_frame(torch, ctx, [synth.synth_motion_frames(NF, NL, 77 * NF + b, CamF, "forward", float_uv=b % 2 == 0) for b in range(B)], 7.0)
    assert n.sum() > 20 * B
    return dict(match=m, nmatches=n)


@case("fuse_search", ["fuse_search"], ((2, 300, 200), (4, 700, 900)))
def _fuse(torch, ctx, B, NF, NP):
    from tests.test_gpu_match import _pack_fuse
    cam = CAM()
    bi, bd = api.fuse_search(ctx, cam, *_pack_fuse(torch, [synth.synth_fuse_frame(NF, NP, 800 + NF + i, float_coords=i % 2 == 0) for i in range(B)]), th=3.0)
    out = H(torch, dict(best_idx=bi, best_dist=bd))
    assert (out["best_idx"] >= 0).sum() > 20 * B
    return out


def _pairs(big):
    sizes = ((700, 900, 25), (300, 350, 60), (1200, 1100, 200)) if big else ((64, 70, 5), (30, 41, 5))
    return sizes


@case("search_for_triangulation_gather", ["search_for_triangulation", "gather_triangulation_matches"], ((False,), (True,)))
def _tri(torch, ctx, big):
    from tests.test_gpu_match import _pack_pairs
    cam, K = CAM(), 5
    mean, _ = map_v1()
    rng = np.random.default_rng(3)
    pairs = [synth.synth_tri_search_pair(N1, N2, 400 + i + N1, cam, n_nodes=nodes, pad=1) for i, (N1, N2, nodes) in enumerate(_pairs(big))]
    k1, k2, fm, ep = _pack_pairs(torch, pairs)
    match, nm = api.search_for_triangulation(ctx, k1, k2, fm, ep, False, True)

    def side(key, pose_key, N):  # depth, candidate components per feature (kf->comps_), the pose: what createMapPoints takes per match
        t = dict(pose=np.zeros((len(pairs), 7)), uv=np.zeros((len(pairs), N, 2)), ur=np.full((len(pairs), N), -1.0, np.float32),
                 depth=np.full((len(pairs), N), -1.0, np.float32), oct=np.zeros((len(pairs), N), np.int32), cand=np.full((len(pairs), N, K), -1, np.int32),
                 ncand=np.zeros((len(pairs), N), np.int32))
        for b, p in enumerate(pairs):
            k = p[key]
            n = len(k["oct"])
            t["pose"][b] = p[pose_key]
            t["uv"][b, :n], t["ur"][b, :n], t["oct"][b, :n] = k["uv"], k["ur"], k["oct"]
            t["depth"][b, :n] = np.where(k["ur"] >= 0, cam.bf / np.maximum(k["uv"][:, 0] - k["ur"], 1e-3), -1.0)
            t["cand"][b, :n] = rng.integers(0, mean.shape[0], (n, K))
            t["ncand"][b, :n] = rng.integers(0, K + 1, n)
        return {q: T(torch, v) for q, v in t.items()}
    off, m = api.gather_triangulation_matches(ctx, match, nm, side("kf1", "pose1", match.shape[1]), side("kf2", "pose2", k2["oct"].shape[1]))
    out = H(torch, dict(m, match=match, nmatches=nm, pair_off=off))
    assert out["nmatches"].sum() > (100 if big else 8) and out["pair_off"][-1] == out["nmatches"].sum()
    return out


@case("search_by_bow", ["search_by_bow"], ((False,), (True,)))
def _bow(torch, ctx, big):
    from tests.test_gpu_match import _pack_bow
    pairs = [synth.synth_bow_pair(N1, N2, 600 + i + N1, CAM(), n_nodes=nodes) for i, (N1, N2, nodes) in enumerate(_pairs(big))]
    match, nm = api.search_by_bow(ctx, *_pack_bow(torch, pairs), 0.7, True)
    out = H(torch, dict(match=match, nmatches=nm))
    assert out["nmatches"].sum() > (100 if big else 8)
    return out


@functools.lru_cache(maxsize=None)
def _local_points_frames(B, NF, NP):
    return [synth.synth_local_points_frame(NF, NP, 3000 + NF + i, CAM(), float_uv=i % 3 != 0) for i in range(B)]


PROJ_KEYS = ("pose_cw", "t_wc", "pos", "normal", "max_dist", "min_dist", "cand")


@case("project_map_points", ["project_map_points"], ((2, 300, 700), (4, 900, 2500)))
def _project(torch, ctx, B, NF, NP):
    from tests.test_gpu_match import _pack_project
    res = api.project_map_points(ctx, CAM(), *_pack_project(torch, _local_points_frames(B, NF, NP)))
    out = H(torch, dict(zip(("uvr", "level", "viewcos", "dist", "inview"), res)))
    assert out["inview"].sum() > 50 * B
    return out


def _slp_inputs(torch, frames):
    from tests.test_gpu_match import _pack_project
    feat = [T(torch, np.stack([f[k] for f in frames])) for k in ("feat_uv", "feat_ur", "feat_oct", "feat_desc", "feat_taken")]
    return feat, _pack_project(torch, frames), T(torch, np.stack([f["mp_desc"] for f in frames]))


@case("search_local_points", ["search_local_points"], ((2, 300, 700), (4, 900, 2500)),
      check=lambda oracle, out: _check_search_local_points(oracle, out))
def _slp(torch, ctx, B, NF, NP):
    feat, proj, desc = _slp_inputs(torch, _local_points_frames(B, NF, NP))
    match, nm, inview = api.search_local_points(ctx, CAM(), *feat, *proj, desc, th=3.0)
    out = H(torch, dict(match=match, nmatches=nm, inview=inview))
    assert out["nmatches"].sum() > 20 * B
    return out


def _check_search_local_points(oracle, out, B=2, NF=300, NP=700):
    """the assertions of tests/test_gpu_match.py::test_search_local_points_chain_matches_oracle"""
    cam = CAM()
    for b, f in enumerate(_local_points_frames(B, NF, NP)):
        uvr, lvl, vc, dd, iv, n = oracle.project_map_points(cam, **{k: f[k] for k in PROJ_KEYS})
        ref, nref = oracle.search_by_projection(cam.width, cam.height, f["feat_uv"], f["feat_ur"], f["feat_oct"], f["feat_desc"], f["feat_taken"], uvr, lvl, vc,
                                                iv, f["mp_desc"], th=3.0)
        assert np.array_equal(out["inview"][b], iv), b
        assert np.array_equal(out["match"][b], ref) and out["nmatches"][b] == nref, (b, int((out["match"][b] != ref).sum()))


# ---------------------------------------------------------------------------------------------------------------- the resident map
@case("update_map_points", ["update_map_points"], ((40,), (3000,)))
def _update_map_points(torch, ctx, extra):
    from tests.test_gpu_map_points import mixed_map, sentinel
    m = mixed_map(11, extra=extra)
    NP = len(m["mp"]["obs_ptr"]) - 1
    o = to_dev(torch, sentinel(NP))
    api.update_map_points(ctx, to_dev(torch, m["kf"]), to_dev(torch, m["mp"]), o)
    out = H(torch, o)
    assert (out["desc"] != 0xA5).any(1).sum() > NP // 2
    return out


@functools.lru_cache(maxsize=None)
def _update_scene(name):
    return LS.update_scene(name)


def _update_local_map(torch, ctx, name, B, with_count):
    from tests.test_gpu_local_map import device_update
    m, feat_mp, lists = _update_scene(name)
    lists = {k: v[:B] for k, v in lists.items() if with_count or k != "kf_count"}
    fm, ls = device_update(torch, ctx, m, feat_mp[:B], lists)
    assert (ls["status"] == 0).any() and (ls["n_local_mp"] > 5).any()
    return dict(ls, feat_mp=fm)


case("update_local_map", ["update_local_map"], (("tiny", 16, True), ("small", 24, True)))(_update_local_map)
# more than 4 096 key-frames and no kf_count of the caller's: the per-frame counters live in the context's block
case("update_local_map_counters_in_scratch", ["update_local_map"], (("kf_over_bound", 3, False), ("kf_over_bound", 16, False)))(_update_local_map)


@functools.lru_cache(maxsize=None)
def _window_scene(name):
    return BS.scene(name)


def _update_connections(torch, ctx, name, B, with_count):
    from tests.test_gpu_ba_window import conn_out, device_connections
    m, ba, rows = _window_scene(name)
    out = device_connections(torch, ctx, to_dev(torch, m), rows[:B], conn_out(B, 64, m["kf_mp"].shape[0] if with_count else None))
    assert (out["n_conn"] >= 1).sum() >= B - 2 and (out["conn_w"][:, 0] > 0).sum() >= B - 2, out["n_conn"]  # (every window of `tiny` lists its single largest)
    return out


case("update_connections", ["update_connections"], (("tiny", 16, True), ("small", 16, True)))(_update_connections)
case("update_connections_counters_in_scratch", ["update_connections"], (("kf_over_bound", 3, False), ("kf_over_bound", 16, False)))(_update_connections)


@functools.lru_cache(maxsize=None)
def _window_ref(name):
    m, ba, rows = _window_scene(name)
    _, wins = BR.ba_window_build(m, ba, rows, BS.empty_slab(len(rows), (1, 1, 1, 1)))
    caps = BS.caps_of(wins)
    built, _ = BR.ba_window_build(m, ba, rows, BS.empty_slab(len(rows), caps))
    return caps, built


@case("ba_window_build", ["ba_window_build"], (("tiny",), ("small",)))
def _ba_window_build(torch, ctx, name):
    from tests.test_gpu_ba_window import device_build
    m, ba, rows = _window_scene(name)
    out = device_build(torch, ctx, to_dev(torch, m), to_dev(torch, ba), rows, BS.empty_slab(len(rows), _window_ref(name)[0]))
    assert (out["sizes"][:, 2] > 0).any() and not (out["status"] & BR.TRUNCATED).any()
    return out


@case("ba_window_apply", ["ba_window_apply"], (("tiny",), ("small",)))
def _ba_window_apply(torch, ctx, name):
    from tests.test_gpu_ba_window import fake_ba_outputs
    m, ba, rows = _window_scene(name)
    slab, dropped, erase, iters = fake_ba_outputs(_window_ref(name)[1], np.random.default_rng(9))
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    B, Ocap = erase.shape
    sd = to_dev(torch, dict(slab, dropped=dropped, erase=erase, iters=iters, erase_obs=np.full((B, Ocap), -7, np.int32), n_erase=np.full(B, -7, np.int32)))
    eo, ne = api.ba_window_apply(ctx, md, bd, sd)
    out = H(torch, dict(kf_pose=bd["kf_pose"], kf_twc=bd["kf_twc"], mp_pos=md["mp_pos"], mp_assoc=bd["mp_assoc"], erase_obs=eo, n_erase=ne))
    assert (out["n_erase"] > 1).any() and not np.array_equal(out["mp_assoc"], ba["mp_assoc"])
    return out


GEO_LARGE = dict(NKF=36, NFK=300, per_kf=150)  # twice the points and slots per key-frame of tests/ba_window_scenes.py::GEO


@functools.lru_cache(maxsize=None)
def _geo_scene(big):
    saved = dict(BS.GEO)
    try:
        if big:
            BS.GEO.update(GEO_LARGE)
        m, ba, kf = BS.geometric_scene(*map_v1(), gt_sync()["V1_01_easy"], CAM())
    finally:
        BS.GEO.clear()
        BS.GEO.update(saved)
    rng = np.random.default_rng(8)
    ba_clamped = dict(ba, kf_oct=np.minimum(ba["kf_oct"], 1).astype(np.int32))  # the mapping pass: octaves clamped so that key-frames get culled
    depth = rng.uniform(0.2, 8.0, ba["kf_oct"].shape).astype(np.float32)
    # only the points with at least seven observers keep a depth, so that key-frames ARE culled after the BA's erasures (as
    # tests/test_gpu_map_edit.py::test_mapping_pass_equals_the_host_edits does with five after them) - here by the map on entry: an input
    # fixed before any device call; on the restatement 1 - 5 of the 6 - 7 candidates are culled with a tenth to a fifth of the observations erased
    depth[(ba["kf_uvr"][:, :, 2] < 0) | (m["kf_mp"] < 0) | (np.diff(m["obs_ptr"])[np.maximum(m["kf_mp"], 0)] < 7)] = -1.0
    return m, ba, kf, ba_clamped, depth


# `large`: capacities below the window, so the slab grows once and the window is built twice
GEO_CAPS = {False: (24, 24, 2048, 16384), True: (4, 2, 100, 500)}
SLAB_OUT = BR.WINDOW_ARRAYS + ("sizes", "status", "dropped", "erase", "iters", "erase_obs", "n_erase")


@case("joint_optimization_from_map", ["joint_optimization_from_map"], ((False,), (True,)),
      check=lambda oracle, out: _check_from_map(oracle, out))
def _from_map(torch, ctx, big):
    m, ba, kf, _, _ = _geo_scene(big)
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    r = api.joint_optimization_from_map(ctx, gmm_of(ctx), CAM(), PRM(), md, bd, kf, GEO_CAPS[big])
    out = H(torch, dict({k: r["slab"][k] for k in SLAB_OUT}, kf_pose=bd["kf_pose"], kf_twc=bd["kf_twc"], mp_pos=md["mp_pos"], mp_assoc=bd["mp_assoc"]))
    assert out["iters"][0] > 0 and out["n_erase"][0] > 0 and (not big or r["caps"] != GEO_CAPS[big])
    return out


def _check_from_map(oracle, out):
    """tests/test_gpu_ba_window.py::test_joint_optimization_from_map_equals_the_uploaded_window, without the GPU in the reference: the
    window is the restatement's, the BA's outputs within tests/test_gpu_ba.py::check of the oracle's on that window, the resident rows
    the numpy scatter of the slab"""
    from tests.test_gpu_ba import check as ba_check
    m, ba, kf, _, _ = _geo_scene(False)
    w = BR.window_vec(m, ba, kf)
    P, F, L, nobs = w["P"], w["F"], w["L"], w["nobs"]
    assert out["sizes"][0].tolist() == [P, F, L, nobs] and not out["status"][0] & BR.TRUNCATED
    assert np.array_equal(out["win_kf"][0, :P + F], w["win_kf"]) and np.array_equal(out["win_mp"][0, :L], w["win_mp"])
    prob = dict(P=P, F=F, poses=w["poses"], prior=w["prior"], points=w["points"], obs_ptr=w["obs_ptr"], obs_pose=w["obs_pose"], obs_uvr=w["obs_uvr"],
                obs_oct=w["obs_oct"])
    h = oracle.gmm_create(*map_v1())
    ba_check([prob], [w["assoc"]], [out["poses"][:, :P + F], out["points"][:, :L], out["dropped"][:, :L], out["erase"][:, :nobs], out["iters"]], oracle, h, CAM())
    oracle.gmm_destroy(h)
    before = dict(kf_pose=ba["kf_pose"], kf_twc=ba["kf_twc"], mp_pos=m["mp_pos"], mp_assoc=ba["mp_assoc"])
    slab = {k: out[k] for k in BR.WINDOW_ARRAYS + ("sizes", "status")}
    ref, lists = BR.ba_window_apply(before, slab, out["dropped"], out["erase"], out["iters"])
    for k in ref:
        assert out[k].tobytes() == ref[k].tobytes(), k
    assert np.array_equal(out["erase_obs"][0, :out["n_erase"][0]], lists[0])


@functools.lru_cache(maxsize=None)
def _edit_scene(name):
    return ES.scene(name, name in ES.CLAMP)


@case("cull_keyframes", ["cull_keyframes"], (("tiny",), ("small",)))
def _cull(torch, ctx, name):
    from tests.test_gpu_map_edit import cull_out, device_cull, lists_of
    sc = _edit_scene(name)
    Ccap = len(sc["cand"]) + 6
    cand, n_cand = lists_of(sc, Ccap)
    out = device_cull(torch, ctx, to_dev(torch, sc["m"]), to_dev(torch, sc["ba"]), sc, cand, n_cand, cull_out(len(cand), Ccap))
    assert out["n_cull"][0] >= 1
    return out


@case("map_remove", ["map_remove"], (("tiny",), ("small",)))
def _remove(torch, ctx, name):
    from tests.test_gpu_map_edit import device_remove
    sc = _edit_scene(name)
    rows, _ = device_remove(torch, ctx, sc, *ES.dirty(sc, *ES.removals(sc, 3)))
    assert rows["n_dead"] > 0 and rows["nobs"] < len(sc["m"]["obs_kf"])
    return {k: np.asarray(v) for k, v in rows.items()}


PASS_KEYS = ("mp_valid", "kf_valid", "kf_mp", "obs_ptr")


@case("mapping_pass_from_map", ["mapping_pass_from_map"], ((False,), (True,)), check=lambda oracle, out: _check_pass(oracle, out))
def _pass(torch, ctx, big):
    m, _, kf, ba, depth = _geo_scene(big)
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    rk = T(torch, ES.first_entry_kf(m))
    p = api.mapping_pass_from_map(ctx, gmm_of(ctx), CAM(), PRM(), md, bd, kf, GEO_CAPS[big], T(torch, depth), ES.TH_DEPTH, mp_ref_kf=rk)
    out = H(torch, dict({k: md[k] for k in PASS_KEYS}, obs_kf=p["map"]["obs_kf"], obs_feat=p["ba_rows"]["obs_feat"], mp_ref_kf=rk, kf_pose=bd["kf_pose"],
                        mp_pos=md["mp_pos"], mp_assoc=bd["mp_assoc"], cull=p["cull"]["cull"], conn_kf=p["conn"]["conn_kf"], n_conn=p["conn"]["n_conn"]))
    for k in ("erased", "dead_by_erase", "culled", "dead_by_cull", "status"):
        out[k] = np.asarray(p[k], np.int64)
    assert len(p["erased"]) > 0 and len(p["culled"]) >= 1 and out["n_conn"][0] >= 1, (len(p["erased"]), p["culled"], out["n_conn"])
    return out


def _check_pass(oracle, out):
    """tests/test_gpu_map_edit.py::test_mapping_pass_equals_the_host_edits from the pass's own erase list on: the restatement's erase /
    connections / cull / remove on the host's rows give the map's arrays and the bookkeeping lists bit for bit"""
    m, _, kf, ba, depth = _geo_scene(False)
    ref_kf = ES.first_entry_kf(m)
    rows1, _ = ER.map_remove(m, ba, erase_obs=out["erased"].astype(np.int32), mp_ref_kf=ref_kf)
    m1, ba1 = ER.apply_rows(m, ba, rows1)
    cand = BR.connections_vec(m1, kf)["conn_kf"][:64]
    cull = ER.Model(m1, ba1).remove_key_frames(cand, depth, ES.TH_DEPTH)
    rows2, _ = ER.map_remove(m1, ba1, rm_kf=cull["cull_rows"], mp_ref_kf=rows1["mp_ref_kf"])
    assert out["dead_by_erase"].tolist() == rows1["dead_mp"].tolist() and out["culled"].tolist() == cull["cull_rows"].tolist()
    assert out["dead_by_cull"].tolist() == rows2["dead_mp"].tolist() and out["status"].tolist() == [0, 0]
    for k in PASS_KEYS + ("obs_kf", "obs_feat", "mp_ref_kf"):
        a, b = out[k], np.asarray(rows2[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert np.array_equal(out["cull"][0, :len(cand)], cull["cull"])


# ---------------------------------------------------------------------------------------------------------------- the tracked frame
@functools.lru_cache(maxsize=None)
def _chain_frames(big):
    cam = CAM()
    if not big:
        return [synth.synth_chain_frame(300, 250, 600, 5900 + b, cam, NK=200, temporal_frac=(0.2 if b == 1 else 0.0)) for b in range(2)]
    # 1 400 local map points, one frame 10 degrees off its prediction: through the key-frame fallback
    return [synth.synth_chain_frame(700, 600, 1400, 5700 + b, cam, NK=500, temporal_frac=(0.2 if b == 2 else 0.0), pred_rot_deg=(10.0 if b == 1 else None))
            for b in range(3)]


def _chain_nontrivial(out, big):
    assert (out["counts"][:, 2] > 0).any() and (out["counts"][:, 3] > 10).any()
    assert out["counts2"][:, 3].tolist() == ([0, 1, 0] if big else [0, 0])


@case("track_frame_chain", ["track_frame_chain"], ((False,), (True,)), check=lambda oracle, out: _check_chain(oracle, out))
def _chain(torch, ctx, big):
    from tests.test_gpu_chain import run_chain
    out = run_chain(torch, ctx, _chain_frames(big))
    _chain_nontrivial(out, big)
    return out


@case("track_frame_chain_halves", ["track_frame_chain_front", "track_frame_chain_back"], ((False,), (True,)), check=lambda oracle, out: _check_chain(oracle, out))
def _chain_halves(torch, ctx, big):
    from tests.test_gpu_chain import pack
    a = pack(torch, _chain_frames(big))
    front = api.track_frame_chain_front(ctx, CAM(), PRM(), a, th_mm=TH_MM)
    out = H(torch, api.track_frame_chain_back(ctx, CAM(), PRM(), a, front, th_local=TH_LOCAL, nn_ratio=0.8))
    _chain_nontrivial(out, big)
    return out


def _check_chain(oracle, out, frames=None):
    for b, f in enumerate(frames or _chain_frames(False)):
        G.check_chain(oracle, CAM(), f, out, b)


@functools.lru_cache(maxsize=None)
def _chain_map_scene(big):
    """tests/local_map_scenes.py::chain_scene for the frames above, without invalid map points (check_chain knows no clearing)"""
    frames = _chain_frames(big)
    NKF, NFK, KFcap, NPcap = (300, 1000, 64, 1728) if big else (120, 500, 64, 960)
    NMP = int(sum(len(f["mp_cand"]) for f in frames) * 1.3) + 64
    s = synth.synth_chain_map(frames, 25 + big, NMP, NKF, NFK, pt_invalid_frac=0.0)
    lists = LS.previous_lists(len(frames), NKF, NMP, KFcap, NPcap)
    for b in range(len(frames)):
        n, k = min(len(s["prev_local_mp"][b]), NPcap), min(len(s["prev_local_kf"][b]), KFcap)
        lists["local_mp"][b, :n], lists["n_local_mp"][b] = s["prev_local_mp"][b][:n], n
        lists["local_kf"][b, :k], lists["n_local_kf"][b] = s["prev_local_kf"][b][:k], k
    return frames, s, lists, NPcap


@case("track_frame_chain_map", ["track_frame_chain_map"], ((False,), (True,)), check=lambda oracle, out: _check_chain_map(oracle, out))
def _chain_map(torch, ctx, big):
    from tests.test_gpu_local_map import run_map_chain
    frames, s, lists, NPcap = _chain_map_scene(big)
    out, ls = run_map_chain(torch, ctx, frames, s, lists, NPcap)
    _chain_nontrivial(out, big)
    assert (ls["status"] == 0).all() and (ls["n_local_mp"] > 100).all(), (ls["status"], ls["n_local_mp"])
    return dict(out, **ls)


def _check_chain_map(oracle, out):
    """tests/test_gpu_local_map.py::test_chain_map_stages_equal_the_oracle_on_the_device_made_list"""
    frames, s, lists, NPcap = _chain_map_scene(False)
    for b, f in enumerate(frames):
        g = dict(f)
        g.update(LR.gather_local_map(s["map"], out["local_mp"][b], out["n_local_mp"][b], NPcap, s["last_mp"][b], s["kf_feat_mp"][b]))
        G.check_chain(oracle, CAM(), g, out, b)
        r = LR.frame_vec(s["map"], out["feat_mp"][b])
        assert np.array_equal(r["local_mp"], out["local_mp"][b, :out["n_local_mp"][b]]) and r["ref_kf"] == out["ref_kf"][b]


BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the cases the timing / statistics leg runs
TIMING_CASES = ("track_frames_batch_shape", "track_frames_latency_shape", "optimize_current_pose", "joint_optimization", "track_frame_chain")
