"""CPU: the C++ oracle against the independent numpy restatement (oracle/numpy_ref.py) AWAY from the default camera and
parameters (tests/configs.py), computed live at small sizes, at the tolerances test_oracle_golden.py holds for the same pair;
and the power check: for every function and every mutation of a field it reads ("swap fx / fy", "swap tri_lambda2 / ba_lambda2",
"the default gl_params", "scale factor 1.2") the oracle's own output moves by at least 100 x the tolerance the GPU test holds
for it, or by at least one element of an integer output - so a kernel that reads the wrong field cannot pass the GPU tests of
tests/test_gpu_configs.py.

READS says which fields each function reads; a mutation that changes none of them for a configuration is not applied there
(e.g. "swap fx / fy" under WIDE, whose camera is isotropic; render_view reads no parameter at all)."""
import numpy as np
import pytest

from gmmloc_amd import synth
from tests.configs import CONFIGS, MUTATIONS
from tests.test_gpu_pose import make_frames, pose_err

import numpy_ref as nr  # noqa: E402  (tests.configs puts oracle/ on the path)

CAM, PIX, IMG = ("fx", "fy", "cx", "cy"), ("fx", "fy", "cx", "cy", "bf"), ("width", "height")
TRI = ("tri_lambda2", "tri_str_thresh", "tri_check_str_chi2", "sigma2_inv")
READS = {
    "render_view": CAM + IMG,
    "optimize_point": PIX + TRI,
    "check_map_association": PIX + TRI + ("neighbor_dist_thresh",),
    "optimize_triangulation": PIX + TRI,
    "create_map_points": PIX + TRI + ("scale_factor",),
    "optimize_current_pose": PIX + ("sigma2_inv",),
    "joint_optimization": PIX + ("ba_lambda2", "tri_str_thresh", "ba_first_as_prior", "sigma2_inv"),
    "neighbour_rows": ("neighbor_dist_thresh",),
    "search_by_projection": IMG + ("scale_factor",),
    "search_by_projection_frame": PIX + IMG + ("scale_factor",),
    "fuse_search": IMG + ("scale_factor",),
    "project_map_points": PIX + IMG + ("scale_factor",),
    "search_for_triangulation": ("scale_factor",),
}
# the tolerances of the GPU parity tests (test_gpu_pose / _track / _ba: 1e-6 m, 1e-6 rad; test_gpu_view_point: 1e-9 on points,
# 1e-8 on the points of create_map_points); the power check asks for 100 x these
TOL_POSE, TOL_POINT, TOL_CMP = 1e-6, 1e-9, 1e-8
POWER = 100.0


def field(cfg, k):
    if k == "sigma2_inv":
        return tuple(cfg.sigma2_inv.tolist())
    if k == "scale_factor":
        return cfg.scale_factor
    return cfg.cam[k] if k in cfg.cam else cfg.prm[k]


ALL4 = {"swap_fx_fy", "swap_lambdas", "default_params", "scale_1.2"}
# which mutations must apply to which function, written out by hand (not derived from READS): ANISO differs from the defaults in
# every field; NOSTR in the lambdas, the threshold and the switch only (default camera, 1.2 pyramid); WIDE in the camera only, an
# isotropic one - no mutation changes anything there
EXPECTED = {
    "ANISO": {"render_view": {"swap_fx_fy"}, "optimize_point": ALL4, "check_map_association": ALL4, "optimize_triangulation": ALL4,
              "create_map_points": ALL4, "optimize_current_pose": {"swap_fx_fy", "default_params", "scale_1.2"}, "joint_optimization": ALL4,
              "neighbour_rows": {"default_params"}, "search_by_projection": {"scale_1.2"},
              "search_by_projection_frame": {"swap_fx_fy", "scale_1.2"}, "fuse_search": {"scale_1.2"},
              "project_map_points": {"swap_fx_fy", "scale_1.2"}, "search_for_triangulation": {"scale_1.2"}},
    "NOSTR": {fn: {"swap_lambdas", "default_params"} for fn in ("optimize_point", "check_map_association", "optimize_triangulation",
                                                                 "create_map_points", "joint_optimization")},
    "WIDE": {},
}


def mutants(cfg, fn):
    """(name, mutated configuration) for every mutation that changes a field `fn` reads under `cfg`; the set is checked against
    EXPECTED, so that a function cannot drop out of the power check through a slip in READS"""
    out = []
    for name, mut in MUTATIONS.items():
        m = mut(cfg)
        if any(field(m, k) != field(cfg, k) for k in READS[fn]):
            out.append((name, m))
    assert {name for name, _ in out} == EXPECTED[cfg.name].get(fn, set()), (cfg, fn, [name for name, _ in out])
    return out


@pytest.fixture(scope="module")
def world(map_v1, gt_sync):
    mean, cov = map_v1
    seq = gt_sync["V1_01_easy"]
    return dict(mean=mean, cov=cov, comps=nr.build_components(mean, cov), seq=seq,
                poses=np.stack([synth.gt_row_to_Tcw(seq[i]) for i in (50, 900, 2100)]))


@pytest.fixture
def h(oracle, map_v1):
    # a handle per test: the oracle builds its neighbour graph once per handle, at the threshold of the first call
    hh = oracle.gmm_create(*map_v1)
    yield hh
    oracle.gmm_destroy(hh)


def pose_move(a, b):
    return max(pose_err(a, b))


def record(fn, cfg, mut, margin, unit="x the required movement"):
    """the observed margin of one (function, configuration, mutation), printed (pytest -s): the docstrings quote the smallest"""
    print("power %-28s %-6s %-15s %12.1f %s" % (fn, cfg.name, mut, margin, unit))


# ------------------------------------------------------------------ A3-A5
@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_render_view_and_search(oracle, h, world, cfg):
    """A3-A5 as test_oracle_golden.test_render_view_and_search: the rendered ids in depth order and the k = 5 candidates, exact.
    Power (ANISO, swap fx / fy): smallest observed change 298 rendered ids / candidate slots."""
    W, H = cfg.cam["width"], cfg.cam["height"]
    rng = np.random.default_rng(5)
    uv = np.stack([rng.uniform(0, W, 150), rng.uniform(0, H, 150)], 1)

    def run(c, pose):
        ids, m2, c2, dep = oracle.render_view(h, c.camlike(), pose)
        cand, ncand = oracle.search_correspondence(h, uv, 5)
        return ids, cand, ncand, dep, c2
    for pose in world["poses"][:2]:
        ids, cand, ncand, dep, c2 = run(cfg, pose)
        view = nr.render_view(world["mean"], world["cov"], world["comps"], cfg.np_cam(), pose)
        assert np.array_equal(ids, np.array([g["id"] for g in view], np.int32))
        assert (np.diff(dep) <= 0).all() and (np.linalg.eigvalsh(c2.reshape(-1, 2, 2)) > 0).all()
        c_ref, n_ref = nr.search_correspondence(view, uv, 5)
        assert np.array_equal(ncand, n_ref) and np.array_equal(cand, c_ref)
        assert len(ids) > 50
        for name, m in mutants(cfg, "render_view"):
            ids_m, cand_m, ncand_m, _, _ = run(m, pose)
            changed = int((cand_m != cand).sum()) + (len(ids_m) != len(ids) or int((ids_m != ids).sum()))
            assert changed >= 1, name
            record("render_view", cfg, name, changed, "elements")


# ------------------------------------------------------------------ B1 / A8 / B2 / createMapPoints
def point_inputs(world, cfg, N=60):
    """the inputs of make_golden.py's B1 / A8 / B2 sections under the configuration's camera"""
    mean, cov, comps, cam = world["mean"], world["cov"], world["comps"], cfg.camlike()
    # (the second key-frame is a neighbour of the first: every point is in front of both, so that Gauss-Newton on a far-away
    # candidate plane - which tri_check_str_chi2 = 0 no longer rejects - stays a well-posed problem)
    pose, pose2 = world["poses"][0], synth.gt_row_to_Tcw(world["seq"][62])
    T = nr.SE3.from7(pose)
    f = synth.synth_frame(mean, cov, pose, cam, N, 77, outlier_frac=0.2, mono_frac=0.0)
    deg = np.nonzero(comps["is_deg"])[0]
    comp = f["comp"].copy()
    comp[~comps["is_deg"][comp]] = deg[0]
    # every 6th point is observed, noise-free, 0.1 - 0.5 m off its plane: the optimum keeps a small reprojection error and a
    # structure chi2 above tri_str_thresh * tri_lambda2 - the points on which tri_check_str_chi2 alone decides
    off = np.arange(0, N, 6)
    f["Xw"][off] += comps["axis"][comp[off]][:, :, 0] * np.random.default_rng(4).uniform(0.1, 0.5, (len(off), 1))
    f["obs"][off] = np.array([nr.proj_stereo(T.map(x), cfg.np_cam()) for x in f["Xw"][off]])
    pz = np.minimum(1.0, T.map(f["Xw"])[:, 2]) ** 2
    X0 = f["Xw"] + np.random.default_rng(3).standard_normal((N, 3)) * 0.02
    rng8 = np.random.default_rng(18)
    K = mean.shape[0]
    cands = -np.ones((N, 5), np.int32)
    for i in range(N):
        n = int(rng8.integers(0, 5))
        c = [int(f["comp"][i])] + [int(x) for x in rng8.integers(0, K, 4)]
        rng8.shuffle(c)
        cands[i, :n] = c[:n]
    T2 = nr.SE3.from7(pose2)
    pc2 = np.array([T2.map(x) for x in f["Xw"]])
    u2 = cam.fx * pc2[:, 0] / pc2[:, 2] + cam.cx + rng8.standard_normal(N) * 0.7
    v2 = cam.fy * pc2[:, 1] / pc2[:, 2] + cam.cy + rng8.standard_normal(N) * 0.7
    uvr2 = np.stack([u2, v2, np.where(rng8.uniform(size=N) < 0.5, -1.0, u2 - cam.bf / pc2[:, 2])], 1)
    uvr1 = f["obs"].copy()
    uvr1[rng8.uniform(size=N) < 0.4, 2] = -1.0
    cands2 = -np.ones((N, 5), np.int32)
    for i in range(N):
        n = int(rng8.integers(0, 4))
        cands2[i, :n] = rng8.integers(0, K, n)
    return dict(N=N, pose=pose, pose2=pose2, f=f, comp=comp.astype(np.int32), pz=pz, X0=X0, cands=cands, cands2=cands2, uvr1=uvr1, uvr2=uvr2)


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_optimize_point(oracle, h, world, cfg):
    """B1 as test_oracle_golden.test_optimize_point (result flags exact, estimate 1e-8, chi2 rtol 1e-6).  Under NOSTR the chi2 test
    is off: no point fails for its structure chi2, while the same inputs under tri_check_str_chi2 = 1 do lose some.
    Power: smallest observed movement of an estimate 1.2e6 x the required 100 x 1e-9 m (ANISO, scale factor 1.2)."""
    d = point_inputs(world, cfg)
    N, f = d["N"], d["f"]

    def run(c):
        return oracle.optimize_point(h, c.camlike(), d["X0"], f["obs"], f["octave"], np.tile(d["pose"], (N, 1)), d["comp"], d["pz"],
                                     prm=c.orc_params(oracle))
    res, c2p, c2s, est = run(cfg)
    mean, comps = world["mean"], world["comps"]
    ref = [nr.optimize_point(d["X0"][i], f["obs"][i], int(f["octave"][i]), d["pose"], comps["axis"][d["comp"][i]][:, 0],
                             mean[d["comp"][i]], d["pz"][i], cfg.np_cam(), cfg.np_prm()) for i in range(N)]
    assert np.array_equal(res, np.array([r[0] for r in ref], np.uint8))
    np.testing.assert_allclose(est, np.stack([r[3] for r in ref]), rtol=0, atol=1e-8)
    np.testing.assert_allclose(c2p, np.array([r[1] for r in ref]), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(c2s, np.array([r[2] for r in ref]), rtol=1e-6, atol=1e-9)
    assert 5 < res.sum() < N  # both outcomes
    thr = float(np.float32(np.float32(cfg.prm["tri_str_thresh"]) * np.float32(cfg.prm["tri_lambda2"])))
    if cfg.prm["tri_check_str_chi2"]:
        assert (c2s[res == 0] > thr).any() and not (c2s[res == 1] > thr).any()  # the structure test decides for some
    else:
        assert (c2s[res == 1] > thr).any()  # points the structure test would have failed are kept: the == 0 branch
    for name, m in mutants(cfg, "optimize_point"):
        r = run(m)
        move = np.abs(r[3] - est).max()
        assert move >= POWER * TOL_POINT or (r[0] != res).any(), (name, move)
        record("optimize_point", cfg, name, move / (POWER * TOL_POINT))


def neighbour_lists(world, cfg, need):
    rows = dict(zip(need, [j for j, _ in nr.neighbour_rows(world["mean"], world["cov"], world["comps"]["det"], need,
                                                            thresh=cfg.prm["neighbor_dist_thresh"])]))
    return [rows.get(k, np.zeros(0, int)) for k in range(world["mean"].shape[0])]


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_check_map_association(oracle, map_v1, world, cfg):
    """A8 as test_oracle_golden.test_check_map_association (components exact, points 1e-8), the neighbour refinement walking the
    graph built at the configuration's neighbor_dist_thresh.
    Power: smallest observed movement of a point 5.8e4 x the required 100 x 1e-9 m (ANISO, the default gl_params)."""
    d = point_inputs(world, cfg)
    N, f = d["N"], d["f"]

    def run(c):
        hh = oracle.gmm_create(*map_v1)  # (the neighbour graph is built once per handle)
        try:
            return oracle.check_map_association(hh, c.camlike(), d["pose"], d["X0"], f["obs"], f["octave"], d["cands"],
                                                (d["cands"] >= 0).sum(1).astype(np.int32), prm=c.orc_params(oracle))
        finally:
            oracle.gmm_destroy(hh)
    out, pts = run(cfg)
    nbs = neighbour_lists(world, cfg, sorted(set(int(c) for c in d["cands"].ravel() if c >= 0)))
    ref = [nr.check_map_association(d["X0"][i], f["obs"][i], int(f["octave"][i]), d["pose"], d["cands"][i], world["comps"], world["mean"],
                                    nbs, cfg.np_cam(), cfg.np_prm()) for i in range(N)]
    assert np.array_equal(out, np.array([r[0] for r in ref], np.int32))
    np.testing.assert_allclose(pts, np.array([r[1] for r in ref]), rtol=0, atol=1e-8)
    assert (out >= 0).sum() > 5
    for name, m in mutants(cfg, "check_map_association"):
        o, p = run(m)
        move = np.abs(p - pts).max()
        assert move >= POWER * TOL_POINT or (o != out).any(), (name, move)
        record("check_map_association", cfg, name, move / (POWER * TOL_POINT))


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_optimize_triangulation(oracle, h, world, cfg):
    """B2 as test_oracle_golden.test_optimize_triangulation (components exact, points 1e-8).
    Power: smallest observed movement of a point 8.1e4 x the required 100 x 1e-9 m (ANISO, the default gl_params)."""
    d = point_inputs(world, cfg)
    N, f = d["N"], d["f"]
    n1, n2 = (d["cands"] >= 0).sum(1).astype(np.int32), (d["cands2"] >= 0).sum(1).astype(np.int32)

    def run(c):
        return oracle.optimize_triangulation(h, c.camlike(), d["X0"], np.tile(d["pose"], (N, 1)), d["uvr1"], f["octave"],
                                             np.tile(d["pose2"], (N, 1)), d["uvr2"], f["octave"], d["cands"], n1, d["cands2"], n2,
                                             prm=c.orc_params(oracle))
    out, x = run(cfg)
    ref = [nr.optimize_triangulation(d["X0"][i], d["pose"], d["uvr1"][i], int(f["octave"][i]), d["pose2"], d["uvr2"][i], d["cands"][i],
                                     d["cands2"][i], world["comps"], world["mean"], cfg.np_cam(), cfg.np_prm()) for i in range(N)]
    assert np.array_equal(out, np.array([r[0] for r in ref], np.int32))
    np.testing.assert_allclose(x, np.array([r[1] for r in ref]), rtol=0, atol=1e-8)
    assert 5 < (out >= 0).sum() < N
    for name, m in mutants(cfg, "optimize_triangulation"):
        o, p = run(m)
        move = np.abs(p - x).max()
        assert move >= POWER * TOL_POINT or (o != out).any(), (name, move)
        record("optimize_triangulation", cfg, name, move / (POWER * TOL_POINT))


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_create_map_points(oracle, h, world, cfg):
    """createMapPoints per-match block as test_oracle_golden.test_create_map_points (types exact; components and points, 1e-7, of
    the matches that reached B2), at the configured scale factor (the ratio test of the two distances).
    Power, on the points alone: smallest observed movement 2.3e5 x the required 100 x 1e-8 m (ANISO, swap fx / fy); 3 - 122 types
    or components change as well."""
    unique_normal = world["comps"]["scale"][:, 1] > 10.0 * world["comps"]["scale"][:, 0]
    seq, NT = world["seq"], 100
    pA, pB = synth.gt_row_to_Tcw(seq[900]), synth.gt_row_to_Tcw(seq[915])
    mt = synth.synth_tri_matches(world["mean"], world["cov"], pA, pB, cfg.camlike(), NT, 91, allowed=unique_normal)

    def run(c):
        return oracle.create_map_points(h, c.camlike(), scale_factor=c.scale_factor, prm=c.orc_params(oracle), **mt)
    x, t, co = run(cfg)
    r_pt, r_type, r_comp = [], [], []
    for i in range(NT):
        pt_i, ty, cc = nr.create_map_point(pA, mt["uvr1"][i], mt["depth1"][i], int(mt["oct1"][i]), pB, mt["uvr2"][i], mt["depth2"][i],
                                           int(mt["oct2"][i]), mt["cand1"][i], mt["cand2"][i], world["comps"], world["mean"], cfg.np_cam(),
                                           cfg.np_prm(), scale_factor=cfg.scale_factor)
        r_pt.append(np.zeros(3) if pt_i is None else pt_i); r_type.append(ty); r_comp.append(cc)
    r_pt, r_type, r_comp = np.array(r_pt), np.array(r_type, np.int32), np.array(r_comp, np.int32)
    assert np.array_equal(t, r_type)
    got = np.abs(r_pt).max(1) > 0
    assert np.array_equal(co[got], r_comp[got])
    np.testing.assert_allclose(x[got], r_pt[got], rtol=0, atol=1e-7)
    assert len(set(t.tolist())) >= 4
    for name, m in mutants(cfg, "create_map_points"):
        xm, tm, cm = run(m)
        # points: where both runs made one, and not the matches that triangulate to points far away (parallel rays: Gauss-Newton is
        # chaotic there, test_gpu_view_point compares only the decision on them)
        both = (t > 0) & (tm > 0) & (np.linalg.norm(x, axis=1) < 100.0)
        move = np.abs(xm - x)[both].max() if both.any() else 0.0
        changed = int((tm != t).sum() + (cm != co).sum())
        assert move >= POWER * TOL_CMP, (name, move)  # (on the points alone; the changed types / components are reported beside it)
        record("create_map_points", cfg, name, move / (POWER * TOL_CMP))
        record("create_map_points", cfg, name, changed, "types / components")


# ------------------------------------------------------------------ B3 / B4
@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
@pytest.mark.parametrize("M,seed", [(60, 11), (200, 12)])
def test_optimize_current_pose(oracle, world, cfg, M, seed):
    """B3 as test_oracle_golden.test_optimize_current_pose (pose 1e-7, outlier mask and inlier count exact); measured agreement
    <= 5e-11 m / 2e-11 rad.  The pose is stable under a permutation of the points (1e-8).
    Power: smallest observed movement of the pose 21.6 x the required 100 x 1e-6 (ANISO, the default gl_params = the 1.2 table
    in place of the 1.25 one)."""
    fr = synth.synth_frame(world["mean"], world["cov"], world["poses"][seed % 3], cfg.camlike(), M, seed)
    if seed % 2:
        fr["octave"][::5] = -1

    def run(c, order=slice(None)):
        return oracle.optimize_current_pose(c.camlike(), fr["pose_init"], fr["Xw"][order], fr["obs"][order], fr["octave"][order],
                                            prm=c.orc_params(oracle))
    p, o, n = run(cfg)
    pr, orf, nrf = nr.optimize_current_pose(fr["pose_init"], fr["Xw"], fr["obs"], fr["octave"], cfg.np_cam(), cfg.np_prm())
    assert pose_move(p, pr) < 1e-7 and np.array_equal(o, orf) and n == nrf
    perm = np.random.default_rng(1).permutation(M)
    pp, op, npn = run(cfg, perm)
    assert pose_move(p, pp) < 1e-8 and np.array_equal(op, o[perm]) and npn == n
    for name, m in mutants(cfg, "optimize_current_pose"):
        move = pose_move(run(m)[0], p)
        assert move >= POWER * TOL_POSE, (name, move)
        record("optimize_current_pose", cfg, name, move / (POWER * TOL_POSE))


# seeds at which the iteration count of the last optimize(40) - rounding noise at convergence, see test_oracle_golden - agrees
# within one under all three configurations (about every second seed does per configuration; the other assertions held on all)
SEEDS = {"track": 33, "window": 32}


def track_problem(world, cfg, M=80, seed=21):
    fr = synth.synth_frame(world["mean"], world["cov"], world["poses"][0], cfg.camlike(), M, seed, outlier_frac=0.08)
    d = nr.chi2_all(world["mean"], world["comps"]["cov_inv"], fr["Xw"])
    a = np.argmin(d, 1)
    assoc = np.where(d[np.arange(M), a] <= 9.0, a, -1).astype(np.int32)
    return dict(P=1, F=0, poses=fr["pose_init"][None], prior=np.zeros(1, np.uint8), points=fr["Xw"], assoc=assoc,
                obs_ptr=np.arange(M + 1, dtype=np.int32), obs_pose=np.zeros(M, np.int32), obs_uvr=fr["obs"], obs_oct=fr["octave"])


def window_problem(world, cfg, L=40, seed=9):
    """3 free + 2 fixed poses, a prior on pose 0, points seen by 2 - 5 poses (make_golden.py's problem (b), one size up)"""
    cam = cfg.np_cam()
    rng = np.random.default_rng(seed)
    base = world["poses"][1]
    Ts = [base] + [synth.perturb_pose(base, rng, 0.02, 0.08) for _ in range(4)]
    fr = synth.synth_frame(world["mean"], world["cov"], base, cfg.camlike(), L, seed + 22, outlier_frac=0.0)
    obs_ptr, obs_pose, obs_uvr, obs_oct = [0], [], [], []
    for l in range(L):
        for pi in range(5):
            if pi >= 2 and (l + pi) % 3 == 0:
                continue
            pc = nr.SE3.from7(Ts[pi]).map(fr["Xw"][l])
            octv = int(rng.integers(0, 4))
            uvr = nr.proj_stereo(pc, cam) + rng.standard_normal(3) * 1.2 ** octv * 0.7
            if (l + pi) % 4 == 0:
                uvr[2] = -1.0
            obs_pose.append(pi); obs_uvr.append(uvr); obs_oct.append(octv)
        obs_ptr.append(len(obs_pose))
    init = np.stack([synth.perturb_pose(Ts[j], rng, 0.003, 0.01) if j < 3 else Ts[j] for j in range(5)])
    d = nr.chi2_all(world["mean"], world["comps"]["cov_inv"], fr["Xw"])
    a = np.argmin(d, 1)
    assoc = np.where(d[np.arange(L), a] <= 9.0, a, -1).astype(np.int32)
    return dict(P=3, F=2, poses=init, prior=np.array([1, 0, 0], np.uint8), points=fr["Xw"] + rng.standard_normal((L, 3)) * 0.01, assoc=assoc,
                obs_ptr=np.array(obs_ptr, np.int32), obs_pose=np.array(obs_pose, np.int32), obs_uvr=np.array(obs_uvr),
                obs_oct=np.array(obs_oct, np.int32))


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
@pytest.mark.parametrize("which", ["track", "window"])
def test_joint_optimization(oracle, h, world, cfg, which):
    joint_case(oracle, h, world, cfg, which, SEEDS[which])


def joint_case(oracle, h, world, cfg, which, seed):
    """B4 as test_oracle_golden.test_joint_optimization (poses 1e-6, dropped associations and erased observations exact, iteration
    count within one, points with a stereo observation 1e-5): the single-pose problem of gl_track_frames (80 points) and a window of
    3 free + 2 fixed poses with a prior.
    Power, on the poses alone: single-pose problem >= 43.5 x the required 100 x 1e-6 (ANISO, swap lambdas: 4.4 mm; swap fx / fy
    5.2e3 x); window >= 6.9 x (NOSTR, swap lambdas; ANISO scale factor 1.2: 8.3 x) - the prior and the fixed poses hold a window's
    poses, so less moves there.  Dropped / erased flags change as well in 7 of the 12 cases."""
    p = track_problem(world, cfg, seed=seed) if which == "track" else window_problem(world, cfg, seed=seed)

    def run(c):
        return oracle.joint_optimization(h, c.camlike(), p["P"], p["F"], p["poses"], p["prior"], p["points"], p["assoc"], p["obs_ptr"],
                                         p["obs_pose"], p["obs_uvr"], p["obs_oct"], prm=c.orc_params(oracle))
    poses, pts, dropped, erase, it = run(cfg)
    r = nr.joint_optimization(p["P"], p["F"], p["poses"], list(p["prior"]), p["points"], p["assoc"], p["obs_ptr"], p["obs_pose"], p["obs_uvr"],
                              p["obs_oct"], world["comps"], world["mean"], cfg.np_cam(), cfg.np_prm())
    for i in range(p["P"]):
        assert pose_move(poses[i], r[0][i]) < 1e-6, i
    assert np.array_equal(dropped, r[2]) and np.array_equal(erase, r[3]) and abs(it - int(r[4])) <= 1
    stereo = np.array([(p["obs_uvr"][p["obs_ptr"][l]:p["obs_ptr"][l + 1], 2] >= 0).any() for l in range(len(pts))])
    assert np.abs(pts - r[1])[stereo].max() < 1e-5
    for name, m in mutants(cfg, "joint_optimization"):
        rm = run(m)
        move = max(pose_move(rm[0][i], poses[i]) for i in range(p["P"]))
        changed = int((rm[2] != dropped).sum() + (rm[3] != erase).sum())
        assert move >= POWER * TOL_POSE, (name, move)  # (on the poses alone; the changed flags are reported beside it)
        record("joint_optimization", cfg, name, move / (POWER * TOL_POSE))
        record("joint_optimization", cfg, name, changed, "dropped / erased flags")


# ------------------------------------------------------------------ A2
@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_neighbour_rows(oracle, h, world, cfg):
    """A2 as test_oracle_golden.test_neighbour_rows (columns exact, distances rtol 1e-8) at the configured threshold.
    Power (ANISO, 1.75 against the default 2.5): 34 fewer neighbours over the 23 rows."""
    rows = list(range(0, 20)) + [1000, 2000, 3298]
    th = cfg.prm["neighbor_dist_thresh"]
    ref = nr.neighbour_rows(world["mean"], world["cov"], world["comps"]["det"], rows, thresh=th)
    tot = 0
    for row, (j, dd) in zip(rows, ref):
        ptr, col, dist = oracle.neighbour_rows(h, row, row + 1, thresh=th)
        assert np.array_equal(col, j), row
        np.testing.assert_allclose(dist, dd, rtol=1e-8, atol=1e-9)
        tot += len(col)
    assert tot > 50
    for name, m in mutants(cfg, "neighbour_rows"):
        tm = sum(len(oracle.neighbour_rows(h, row, row + 1, thresh=m.prm["neighbor_dist_thresh"])[1]) for row in rows)
        assert tm != tot, name
        record("neighbour_rows", cfg, name, abs(tm - tot), "neighbours")


# ------------------------------------------------------------------ the matchers: integer outputs, bit for bit
def power_int(fn, cfg, run, ref_out):
    for name, m in mutants(cfg, fn):
        out = run(m)
        changed = sum(int((np.asarray(a) != np.asarray(b)).sum()) for a, b in zip(out, ref_out))
        assert changed >= 1, (fn, name)
        record(fn, cfg, name, changed, "elements")


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_search_by_projection(oracle, cfg):
    """as test_oracle_golden.test_search_by_projection: matches and count exact, at the configured image size and scale factor.
    Power (ANISO, scale factor 1.2): smallest observed change 26 matches."""
    W, H = cfg.cam["width"], cfg.cam["height"]
    for NF, NP, seed, th in ((250, 300, 101, 3.0), (500, 450, 102, 5.0)):
        fr = synth.synth_match_frame(NF, NP, seed, width=W, height=H, scale_factor=cfg.scale_factor, float_uv=False)
        run = lambda c: oracle.search_by_projection(th=th, scale_factor=c.scale_factor, **dict(fr, width=c.cam["width"], height=c.cam["height"]))
        m, n = run(cfg)
        mr, nrf = nr.search_by_projection(th=th, scale_factor=cfg.scale_factor, **fr)
        assert n == nrf and n > 10 and np.array_equal(m, mr)
        power_int("search_by_projection", cfg, lambda c: run(c)[:1], (m,))


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_search_by_projection_frame(oracle, cfg):
    """as test_oracle_golden.test_search_by_projection_frame, under the configured camera and scale factor.
    Power: smallest observed change 48 matches over the three frames (ANISO, scale factor 1.2)."""
    cases = [(th, synth.synth_motion_frames(NF, NL, seed, cfg.camlike(), motion, float_uv=False))
             for NF, NL, seed, th, motion in ((260, 220, 111, 7.0, "none"), (400, 360, 112, 7.0, "forward"), (380, 400, 113, 14.0, "backward"))]
    run = lambda c: [oracle.search_by_projection_frame(c.camlike(), th=th, scale_factor=c.scale_factor, **fr)[0] for th, fr in cases]
    out = run(cfg)
    for (th, fr), m in zip(cases, out):
        mr, nrf = nr.search_by_projection_frame(cfg.camlike(), th=th, scale_factor=cfg.scale_factor, **fr)
        assert nrf > 20 and np.array_equal(m, mr)
    power_int("search_by_projection_frame", cfg, run, out)


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_fuse_search(oracle, cfg):
    """as test_oracle_golden.test_fuse_search: best feature and distance of every map point exact.
    Power (ANISO, scale factor 1.2): smallest observed change 26 entries."""
    from tests.test_oracle_golden import FUSE_KEYS
    W, H = cfg.cam["width"], cfg.cam["height"]
    for NF, NP, seed, th in ((300, 260, 401, 3.0), (700, 900, 403, 5.0)):
        f = synth.synth_fuse_frame(NF, NP, seed, width=W, height=H, scale_factor=cfg.scale_factor)
        run = lambda c: oracle.fuse_search(*[f[k] for k in FUSE_KEYS], th=th, scale_factor=c.scale_factor)
        bi, bd, n = run(cfg)
        ri, rd, rn = nr.fuse_search(*[f[k] for k in FUSE_KEYS], th=th, scale_factor=cfg.scale_factor)
        assert n == rn and n > 20 and np.array_equal(bi, ri) and np.array_equal(bd, rd)
        power_int("fuse_search", cfg, lambda c: run(c)[:2], (bi, bd))


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_project_map_points(oracle, cfg):
    """as test_oracle_golden.test_project_map_points: every output bit for bit.
    Power: smallest observed change 40 output elements (ANISO, scale factor 1.2)."""
    cam = cfg.camlike()
    for NP, seed in ((400, 501), (1500, 503)):
        f = synth.synth_project_frame(NP, seed, cam, scale_factor=cfg.scale_factor)
        run = lambda c: oracle.project_map_points(c.camlike(), scale_factor=c.scale_factor, **f)
        uvr, lvl, vc, dd, iv, n = run(cfg)
        r = nr.project_map_points(cfg.np_cam(), scale_factor=cfg.scale_factor, **f)
        for a, b in zip((uvr, lvl, vc, dd, iv), r):
            assert np.array_equal(a, b)
        assert n == int(iv.sum()) and 0.1 * NP < n < 0.6 * NP and len(np.unique(lvl[iv > 0])) == 8
        power_int("project_map_points", cfg, lambda c: run(c)[:5], (uvr, lvl, vc, dd, iv))


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_search_for_triangulation(oracle, cfg):
    """as test_oracle_golden.test_search_for_triangulation: matches exact (the epipolar chi2 scales with the level's sigma2).
    Power (ANISO, scale factor 1.2): smallest observed change 1 match of a pair (the scale factor only enters the epipolar gate)."""
    for N1, N2, seed, only_stereo, nodes in ((300, 350, 201, 0, 60), (500, 500, 203, 1, 90), (600, 560, 202, 0, 120)):
        pr = synth.synth_tri_search_pair(N1, N2, seed, cfg.camlike(), n_nodes=nodes, pad=1)
        run = lambda c: oracle.search_for_triangulation(pr["kf1"], pr["kf2"], pr["fmat"], pr["epipole"], bool(only_stereo), True,
                                                        scale_factor=c.scale_factor)
        m, n = run(cfg)
        mr, nrf = nr.search_for_triangulation(pr["kf1"], pr["kf2"], pr["fmat"], pr["epipole"], bool(only_stereo), True, scale_factor=cfg.scale_factor)
        assert n == nrf and n > 15 and np.array_equal(m, mr)
        power_int("search_for_triangulation", cfg, lambda c: run(c)[:1], (m,))


# ------------------------------------------------------------------ the frames of tests/test_gpu_configs.py
def pose_frames(mean, cov, gt, cfg):
    """6 frames of 1 200 feature slots of which 15 - 100 % hold a map point (the reference's frame: compacted where its edges fit)"""
    frames = make_frames(mean, cov, gt["V1_02_medium"], cfg.camlike(), 6, 1200, 9300)
    rng = np.random.default_rng(1200)
    for b, keep in enumerate((0.3, 1.0, 0.45, 0.6, 0.7, 0.15)):
        drop = rng.uniform(size=1200) >= keep
        frames[b]["octave"] = np.where(drop, -1, frames[b]["octave"]).astype(np.int32)
    return frames


def track_frames_of(mean, cov, gt, cfg):
    """two frames of 2 000 points and two small ones (300), one of them with holes"""
    big = make_frames(mean, cov, gt["V1_03_difficult"], cfg.camlike(), 2, 2000, 20, outlier_frac=0.05)
    small = make_frames(mean, cov, gt["V1_03_difficult"], cfg.camlike(), 2, 300, 10, outlier_frac=0.05)
    small[1]["octave"][::7] = -1
    return big, small


@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_gpu_frames_are_stable(oracle, h, map_v1, gt_sync, cfg):
    """No silent exclusions on the GPU: frames exist on which the oracle itself moves under a 1-ulp perturbation
    (tests/test_gpu_soak_cases.py).  pose_frames / track_frames_of (the frames tests/test_gpu_configs.py compares poses
    on) are none of them: the oracle's pose under a permutation of the points stays within 1e-8 on every pose and
    track frame, and on the sparse pose frames (fewer than 400 edges) the numpy restatement agrees with the oracle to the tolerances
    above.  The restatement's un-reduced dense LM takes 30 s on a 300-point track frame, so the track problem is held to it at 80
    points (test_joint_optimization) and not here."""
    from tests.test_gpu_track import oracle_track
    mean, cov = map_v1
    cam, oprm = cfg.camlike(), cfg.orc_params(oracle)
    for i, f in enumerate(pose_frames(mean, cov, gt_sync, cfg)):
        p, o, n = oracle.optimize_current_pose(cam, f["pose_init"], f["Xw"], f["obs"], f["octave"], prm=oprm)
        perm = np.random.default_rng(i).permutation(len(f["octave"]))
        pp, op, npn = oracle.optimize_current_pose(cam, f["pose_init"], f["Xw"][perm], f["obs"][perm], f["octave"][perm], prm=oprm)
        assert pose_move(p, pp) < 1e-8 and npn == n and np.array_equal(op, o[perm]), ("pose", i)
        if (f["octave"] >= 0).sum() < 400:
            pr, orf, nrf = nr.optimize_current_pose(f["pose_init"], f["Xw"], f["obs"], f["octave"], cfg.np_cam(), cfg.np_prm())
            assert pose_move(p, pr) < 1e-7 and np.array_equal(o, orf) and n == nrf, ("pose", i)
    for frames in track_frames_of(mean, cov, gt_sync, cfg):
        for i, f in enumerate(frames):
            keep, p_ref, pts, a_ref, _, _ = oracle_track(oracle, h, cam, f, prm=oprm)
            perm = np.random.default_rng(i).permutation(len(f["octave"]))
            g = {k: (f[k][perm] if k in ("Xw", "obs", "octave") else f[k]) for k in f}
            _, p_perm, _, a_perm, _, _ = oracle_track(oracle, h, cam, g, prm=oprm)
            assert pose_move(p_ref, p_perm) < 1e-8, ("track", len(f["octave"]), i, pose_move(p_ref, p_perm))
