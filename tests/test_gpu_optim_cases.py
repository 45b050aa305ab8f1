"""GPU: every hand-built optimiser case (tests/optim_cases.py) through every launch shape of its kernel.  Integers exactly, what a case
declares unchanged by the bytes, poses and stereo points within 1e-6 of the oracle; each case alone in its call and all cases that can
share a call (one map, one set of parameters) in one batch, padded to a common shape: the same bits (but for bagen_mode 3, the
throughput mode, which is held to the oracle alone).

  gl_optimize_current_pose   pose_waves {0, 1, 4, 8} x pose_regs {0, 1}; pose_compact {0, 1} on 257 slots (245 of them octave -1)
  gl_joint_optimization      bagen_mode 1 with bagen_nb {1, 0}, bagen_mode 2, bagen_mode 3
  gl_track_frames            ba_shape {0, -1, 1} x ba_persist {1, 0}
  gl_track_frames_anchored   on chip: ba_shape {0, -1, 1} x ba_persist {1, 0}, on shape 1 also ba_same_xcd {0, 1}; at the LDS class edges
                             (M = 496, 497, 984, 985, 2000, the case in front of the padding and behind it); packed: by option
                             (ba_fixed_pack = 1), by F (5 and 8, the case's columns first and last), by M (2001); F = 9 is refused

test_float_gap_distance measures the one number the two float cases rest on (see its docstring)."""
import numpy as np
import pytest

import gmmloc_amd
from gmmloc_amd import api
from tests import optim_cases as oc
from tests.test_gpu_pose import pose_err

pytestmark = pytest.mark.gpu
TOL = 1e-6
CAM = oc.camera(oc.CAM5)
_ref = {}


def ref(oracle, name):
    if name not in _ref:
        c = oc.CASES[name]
        _ref[name] = oc.run(oracle, c.call, c.data)
    return _ref[name]


def params(prm):
    return api.Params(**{k: (int(v) if k == "ba_first_as_prior" else float(v)) for k, v in (prm or {}).items()})


def cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- gl_optimize_current_pose ---------------------------------------------------------------------------------------------------------
def run_pose(gpu, datas):
    torch, ctx = gpu
    pose = cuda(torch, np.stack([d["pose"] for d in datas]))
    outl, nin = gmmloc_amd.optimize_current_pose(ctx, CAM, api.Params(), pose, cuda(torch, np.stack([d["Xw"] for d in datas])),
                                                 cuda(torch, np.stack([d["obs"] for d in datas])), cuda(torch, np.stack([d["oct"] for d in datas])))
    torch.cuda.synchronize()
    pose, outl, nin = pose.cpu().numpy(), outl.cpu().numpy(), nin.cpu().numpy()
    return [dict(pose=pose[b], outl=outl[b], nin=int(nin[b])) for b in range(len(datas))]


POSE_M = max(len(oc.CASES[n].data["oct"]) for n in oc.names("pose"))


def check_pose_cases(gpu, oracle, M):
    names = oc.names("pose")
    datas = [oc.pad_rows(oc.CASES[n].data, M) for n in names]
    batch = run_pose(gpu, datas)
    for n, d, o in zip(names, datas, batch):
        c = oc.CASES[n]
        oc.check_declared(c, o, data=d)
        assert not o["outl"][len(c.data["oct"]):].any(), n  # (a slot without a map point is not an outlier)
        assert max(pose_err(o["pose"], ref(oracle, n)["pose"])) < TOL, (n, pose_err(o["pose"], ref(oracle, n)["pose"]))
        one = run_pose(gpu, [d])[0]
        for k in ("pose", "outl", "nin"):
            assert np.array_equal(one[k], o[k]), (n, k, "alone against in the batch")


@pytest.mark.parametrize("regs", [0, 1])
@pytest.mark.parametrize("waves", [0, 1, 4, 8])
def test_pose_cases(gpu, oracle, opt, waves, regs):
    opt("pose_regs", regs)
    opt("pose_waves", waves)
    check_pose_cases(gpu, oracle, POSE_M)


@pytest.mark.parametrize("compact", [0, 1])
def test_pose_cases_on_257_slots(gpu, oracle, opt, compact):
    """pose_compact acts above 256 slots: the twelve edges among 245 slots without a map point, compacted or not"""
    opt("pose_compact", compact)
    check_pose_cases(gpu, oracle, 257)


# ---- gl_joint_optimization ------------------------------------------------------------------------------------------------------------
BA_P, BA_F, BA_L = 2, 4, 12


def ba_groups():
    """the local-BA cases by their parameters; within a group one map: the maps of its cases one after the other, the associations moved up"""
    groups = {}
    for n in oc.names("ba"):
        groups.setdefault(tuple(sorted((oc.CASES[n].data.get("prm") or {}).items())), []).append(n)
    out = []
    for prm, names in sorted(groups.items()):
        means, covs, datas, off = [], [], [], 0
        for n in names:
            d = oc.pad_ba(oc.CASES[n].data, BA_P, BA_F, BA_L)
            d["assoc"] = np.where(d["assoc"] >= 0, d["assoc"] + off, -1).astype(np.int32)
            means.append(np.asarray(d["mean"], float))
            covs.append(np.asarray(d["cov"], float).reshape(-1, 3, 3))
            off += len(means[-1])
            datas.append(d)
        out.append((dict(prm), names, datas, np.concatenate(means), np.concatenate(covs)))
    return out


def run_ba(gpu, g, prm, datas, nobs):
    torch, ctx = gpu

    def pad(a, fill=0):
        out = np.full((nobs,) + a.shape[1:], fill, a.dtype)
        out[:len(a)] = a
        return out

    T = lambda a: cuda(torch, a)
    poses, points = T(np.stack([d["poses"] for d in datas])), T(np.stack([d["points"] for d in datas]))
    dropped, erase, iters = api.joint_optimization(ctx, g, CAM, prm, datas[0]["P"], datas[0]["F"], poses, T(np.stack([d["prior"] for d in datas])), points,
                                                   T(np.stack([d["assoc"] for d in datas])), T(np.stack([d["obs_ptr"] for d in datas])),
                                                   T(np.stack([pad(d["obs_pose"]) for d in datas])), T(np.stack([pad(d["obs_uvr"]) for d in datas])),
                                                   T(np.stack([pad(d["obs_oct"]) for d in datas])))
    torch.cuda.synchronize()
    poses, points, dropped, erase, iters = (x.cpu().numpy() for x in (poses, points, dropped, erase, iters))
    return [dict(poses=poses[b], points=points[b], dropped=dropped[b], erase=erase[b], iters=int(iters[b])) for b in range(len(datas))]


def check_ba(c, o, r, d):
    """o: the device's outputs on d, the case as written or padded; r: the oracle's on the case as written"""
    oc.check_declared(c, o)
    P, L = c.data["P"], len(c.data["points"])
    for j in range(P):
        assert max(pose_err(o["poses"][j], r["poses"][j])) < TOL, (c.name, j, pose_err(o["poses"][j], r["poses"][j]))
    assert o["poses"][P:].tobytes() == d["poses"][P:].tobytes(), (c.name, "a fixed or an unobserved key-frame moved")
    stereo = np.array([(c.data["obs_uvr"][c.data["obs_ptr"][l]:c.data["obs_ptr"][l + 1], 2] >= 0).any() for l in range(L)])
    assert np.abs(o["points"][:L] - r["points"])[stereo].max() < TOL, (c.name, np.abs(o["points"][:L] - r["points"])[stereo].max())
    assert not o["dropped"][L:].any() and not o["erase"][len(c.data["obs_pose"]):].any(), c.name


@pytest.mark.parametrize("mode,nb", [(1, 1), (1, 0), (2, 0), (3, 0)])
def test_ba_cases(gpu, oracle, opt, mode, nb):
    torch, ctx = gpu
    opt("bagen_mode", mode)
    opt("bagen_nb", nb)
    for prm, names, datas, mean, cov in ba_groups():
        g, p = api.GMM(ctx, mean, cov), params(prm)
        nobs = max(len(d["obs_pose"]) for d in datas)
        batch = run_ba(gpu, g, p, datas, nobs)
        for n, d, o in zip(names, datas, batch):
            c = oc.CASES[n]
            check_ba(c, o, ref(oracle, n), d)
            one = run_ba(gpu, g, p, [d], nobs)[0]  # alone, with the batch's shape
            check_ba(c, one, ref(oracle, n), d)
            if mode != 3:
                for k in one:
                    assert np.array_equal(one[k], o[k]), (n, k, "alone against in the batch")
            # and as the case is written, with its own shape and its own map
            own = run_ba(gpu, api.GMM(ctx, np.asarray(c.data["mean"], float), np.asarray(c.data["cov"], float)), p, [c.data], len(c.data["obs_pose"]))[0]
            check_ba(c, own, ref(oracle, n), c.data)


# ---- gl_track_frames ------------------------------------------------------------------------------------------------------------------
def run_track(gpu, g, prm, datas):
    torch, ctx = gpu
    B = len(datas)
    pose, Xw = cuda(torch, np.stack([d["pose"] for d in datas])), cuda(torch, np.stack([d["Xw"] for d in datas]))
    trials, outer = torch.zeros(B, dtype=torch.int32).cuda(), torch.zeros(B, dtype=torch.int32).cuda()
    ctx.set_stats_buffer(trials, outer)
    try:
        assoc, d2 = gmmloc_amd.track_frames(ctx, g, CAM, prm, pose, Xw, cuda(torch, np.stack([d["obs"] for d in datas])), cuda(torch, np.stack([d["oct"] for d in datas])))
        torch.cuda.synchronize()
    finally:
        ctx.set_stats_buffer(None)
    pose, Xw, assoc, d2, outer = (x.cpu().numpy() for x in (pose, Xw, assoc, d2, outer))
    return [dict(pose=pose[b], points=Xw[b], assoc=assoc[b], d2=d2[b], outer=int(outer[b])) for b in range(B)]


@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("shape", [0, -1, 1])
def test_track_cases(gpu, oracle, opt, shape, persist):
    torch, ctx = gpu
    opt("ba_shape", shape)
    opt("ba_persist", persist)
    groups = {}
    for n in oc.names("track"):
        d = oc.CASES[n].data
        groups.setdefault((np.asarray(d["mean"]).tobytes(), np.asarray(d["cov"]).tobytes(), tuple(sorted((d.get("prm") or {}).items()))), []).append(n)
    for names in groups.values():
        d0 = oc.CASES[names[0]].data
        g, p = api.GMM(ctx, np.asarray(d0["mean"], float), np.asarray(d0["cov"], float)), params(d0.get("prm"))
        batch_names = names if len(names) > 1 else names * 2  # (a map of its own: the case twice)
        batch = run_track(gpu, g, p, [oc.CASES[n].data for n in batch_names])
        for n, o in zip(batch_names, batch):
            c, r = oc.CASES[n], ref(oracle, n)
            oc.check_declared(c, o)
            assert max(pose_err(o["pose"], r["pose"])) < TOL, (n, pose_err(o["pose"], r["pose"]))
            assert np.array_equal(o["d2"], r["d2"]), n
            assert np.abs(o["points"] - r["points"]).max() < TOL, (n, np.abs(o["points"] - r["points"]).max())
            one = run_track(gpu, g, p, [c.data])[0]
            for k in one:
                assert np.array_equal(one[k], o[k]), (n, k, "alone against in the batch")


# ---- gl_track_frames_anchored ---------------------------------------------------------------------------------------------------------
def run_anchored(gpu, g, prm, datas, on_chip=True):
    """want_erase = True, the statistics buffer on; `outer` is written by the on-chip route alone"""
    torch, ctx = gpu
    B = len(datas)
    T = lambda k: cuda(torch, np.stack([d[k] for d in datas]))
    pose, Xw = T("pose"), T("Xw")
    trials, outer = torch.zeros(B, dtype=torch.int32).cuda(), torch.zeros(B, dtype=torch.int32).cuda()
    ctx.set_stats_buffer(trials, outer)
    try:
        assoc, d2, fe = gmmloc_amd.track_frames_anchored(ctx, g, CAM, prm, pose, Xw, T("obs"), T("oct"), prior=cuda(torch, np.array([d["prior"] for d in datas], np.uint8)),
                                                         fixed_pose=T("fixed_pose"), fixed_obs=T("fixed_obs"), fixed_oct=T("fixed_oct"), want_erase=True)
        torch.cuda.synchronize()
    finally:
        ctx.set_stats_buffer(None)
    pose, Xw, assoc, d2, fe, outer = (x.cpu().numpy() for x in (pose, Xw, assoc, d2, fe, outer))
    out = [dict(pose=pose[b], points=Xw[b], assoc=assoc[b], d2=d2[b], fixed_erase=fe[b]) for b in range(B)]
    if on_chip:
        for b in range(B):
            out[b]["outer"] = int(outer[b])
    return out


ANC_M = max(len(oc.CASES[n].data["oct"]) for n in oc.names("anchored"))
ANC_F = max(len(oc.CASES[n].data["fixed_pose"]) for n in oc.names("anchored"))
assert ANC_F == 4  # (the on-chip route's limit)


def anchored_groups():
    """the cases that can share a call: one map, one set of parameters"""
    groups = {}
    for n in oc.names("anchored"):
        d = oc.CASES[n].data
        groups.setdefault((np.asarray(d["mean"]).tobytes(), np.asarray(d["cov"]).tobytes(), tuple(sorted((d.get("prm") or {}).items()))), []).append(n)
    return list(groups.values())


def anchored_route(gpu, M, F, where, on_chip):
    """every case padded to M slots and F key-frames, in the batch of its group and alone -> {name: outputs in the case's rows and columns}.
    The same bits alone and in the batch; the padding untouched (unpad_anchored)."""
    torch, ctx = gpu
    out = {}
    for names in anchored_groups():
        d0 = oc.CASES[names[0]].data
        g, p = api.GMM(ctx, np.asarray(d0["mean"], float), np.asarray(d0["cov"], float)), params(d0.get("prm"))
        twins = [n for n in names if "same_as" in oc.CASES[n].want]  # (a twin is a frame of its own, in the batch behind the cases)
        pads = [oc.pad_anchored(oc.CASES[n].data, M, F, where) for n in names] + [oc.pad_anchored(oc.CASES[n].want["same_as"][0], M, F, where) for n in twins]
        batch = run_anchored(gpu, g, p, [x[0] for x in pads], on_chip)
        for i, (n, (d, rows, cols), o) in enumerate(zip(names + [t + " (twin)" for t in twins], pads, batch)):
            if i < len(names):
                one = run_anchored(gpu, g, p, [d], on_chip)[0]
                for k in one:
                    assert np.array_equal(one[k], o[k]), (n, k, "alone against in the batch")
            out[n] = oc.unpad_anchored(o, d, rows, cols)
    return out


def well_held(c, r):
    """the points whose coordinates are compared within TOL: seen in stereo or by a second view that stays, held by the map, or frozen"""
    d = c.data
    well = (d["oct"] >= 0) & ((d["obs"][:, 2] >= 0) | ((d["fixed_oct"] >= 0) & (r["fixed_erase"] == 0)).any(1))
    for l in list(c.want.get("frozen_points", ())) + list(c.want.get("at_mean", {})):
        well[l] = True
    return well


def check_anchored(oracle, res, base=None):
    """the results of one route against the declarations and the oracle, and against another route's (base)"""
    for n in oc.names("anchored"):
        c, o, r = oc.CASES[n], res[n], ref(oracle, n)
        oc.check_declared(c, o)
        assert max(pose_err(o["pose"], r["pose"])) < TOL, (n, pose_err(o["pose"], r["pose"]))
        kept = c.data["oct"] >= 0
        assert np.array_equal(o["d2"][kept], r["d2"][kept]), (n, "d2")
        well = well_held(c, r)
        assert np.abs(o["points"] - r["points"])[well].max() < TOL, (n, np.abs(o["points"] - r["points"])[well].max())
        if "same_as" in c.want:
            oc.check_related(c, o, res[n + " (twin)"])
        if "further_than" in c.want:
            oc.check_related(c, o, res[c.want["further_than"]])
        if base is not None:
            assert np.array_equal(o["assoc"], base[n]["assoc"]) and np.array_equal(o["fixed_erase"], base[n]["fixed_erase"]), (n, "integers across routes")
            assert max(pose_err(o["pose"], base[n]["pose"])) < TOL, (n, "pose across routes", pose_err(o["pose"], base[n]["pose"]))


_anc_base = {}


def anchored_base(gpu, oracle, opt):
    """the route every other one is compared with: on chip, the default launch shape, the cases padded to their common shape alone"""
    if not _anc_base:
        for k, v in (("ba_shape", 0), ("ba_persist", 1), ("ba_same_xcd", 0), ("ba_fixed_pack", 0)):
            opt(k, v)
        _anc_base.update(anchored_route(gpu, ANC_M, ANC_F, "behind", True))
    return _anc_base


@pytest.mark.parametrize("shape,persist,same", [(0, 1, 0), (0, 0, 0), (-1, 1, 0), (-1, 0, 0), (1, 1, 0), (1, 0, 0), (1, 1, 1), (1, 0, 1)])
def test_anchored_cases_on_chip(gpu, oracle, opt, shape, persist, same):
    base = anchored_base(gpu, oracle, opt)
    opt("ba_shape", shape)
    opt("ba_persist", persist)
    opt("ba_same_xcd", same)
    check_anchored(oracle, anchored_route(gpu, ANC_M, ANC_F, "behind", True), base)


def test_anchored_cases_packed_by_option(gpu, oracle, opt):
    base = anchored_base(gpu, oracle, opt)
    opt("ba_fixed_pack", 1)
    check_anchored(oracle, anchored_route(gpu, ANC_M, ANC_F, "behind", False), base)


@pytest.mark.parametrize("where", ["behind", "front"])
@pytest.mark.parametrize("F", [5, 8])
def test_anchored_cases_packed_by_F(gpu, oracle, opt, F, where):
    """more than four fixed key-frames, as a caller reaches the packed route: the case's columns first, or last, among F"""
    check_anchored(oracle, anchored_route(gpu, ANC_M, F, where, False), anchored_base(gpu, oracle, opt))


def test_anchored_cases_packed_by_M(gpu, oracle, opt):
    check_anchored(oracle, anchored_route(gpu, 2001, ANC_F, "behind", False), anchored_base(gpu, oracle, opt))


@pytest.mark.parametrize("where", ["behind", "front"])
@pytest.mark.parametrize("M", [496, 497, 984, 985, 2000])
def test_anchored_cases_at_lds_class_edges(gpu, oracle, opt, M, where):
    check_anchored(oracle, anchored_route(gpu, M, ANC_F, where, True), anchored_base(gpu, oracle, opt))


def test_anchored_nine_fixed_keyframes_are_refused(gpu):
    """F = 9 > GL_TRACK_MAX_FIXED: refused on the host, before any launch, and nothing is written"""
    torch, ctx = gpu
    c = oc.CASES["anc_rho_nonzero"]
    d = oc.pad_anchored(c.data, ANC_M, 9)[0]
    g = api.GMM(ctx, np.asarray(d["mean"], float), np.asarray(d["cov"], float))
    T = lambda k: cuda(torch, d[k][None])
    pose, Xw = T("pose"), T("Xw")
    with pytest.raises(gmmloc_amd.api.GLError, match="fixed observer key-frames"):
        gmmloc_amd.track_frames_anchored(ctx, g, CAM, api.Params(), pose, Xw, T("obs"), T("oct"), prior=cuda(torch, np.ones(1, np.uint8)),
                                         fixed_pose=T("fixed_pose"), fixed_obs=T("fixed_obs"), fixed_oct=T("fixed_oct"), want_erase=True)
    torch.cuda.synchronize()
    assert pose.cpu().numpy().tobytes() == d["pose"].tobytes() and Xw.cpu().numpy().tobytes() == d["Xw"].tobytes()


# ---- the float cases ------------------------------------------------------------------------------------------------------------------
def first_flip(v):
    v = np.asarray(v, int)
    k = np.nonzero(v != v[0])[0]
    assert len(k) and (v[k[0]:] == v[k[0]]).all(), ("the verdict is not one step along the ladder", v)
    return int(k[0])


def test_float_gap_distance(gpu, oracle, opt):
    """pose.float_cast and ba.float_vs_double put a chi2 at 5.991 (1 + 1.5e-8), in the gap of a relative 2.93e-8 between the double 5.991
    and the float 5.991f.  That rests on how far the device's chi2 lies from the oracle's there.  Neither entry point returns a chi2, so the
    distance is read off the verdict: the offset of the case is moved along a ladder of steps of 2^-29 px (a relative 1.52e-9 of chi2),
    and the step at which the device's verdict flips is compared with the oracle's: 36 for the pose optimiser ((float)chi2 > 5.991f:
    half a float ulp above 5.991f) and -9 for the local BA (chi2 > 5.991).  The cases stand while the distance stays within a quarter
    of the gap, 7.3e-9: four steps.
    fx.float_vs_double rests on the same number for a fixed observer's edge of gl_track_frames_anchored, on the on-chip route - which
    evaluates the edge in normalised coordinates - and on the packed one (ba_fixed_pack = 1): read on fixed_erase, the device's verdict
    flips at step -9 on both, as the oracle's: distance 0 steps (below 1.52e-9) each."""
    torch, ctx = gpu
    step = 2 * oc.FLOAT_STEP / oc.D_FLOAT
    out = {}
    for name, ks in (("pose_float_cast", list(range(-12, 60))), ("ba_float_vs_double", list(range(-30, 30))),
                     ("anc_float_vs_double on chip", list(range(-30, 30))), ("anc_float_vs_double packed", list(range(-30, 30)))):
        datas = oc.float_probe(name.split()[0], ks)
        if name.startswith("anc"):  # the fixed edge of column 0 of point 0, through gl_track_frames_anchored on its two routes
            datas = [oc.anchored_from_ba(d)[0] for d in datas]
            g = api.GMM(ctx, np.asarray(datas[0]["mean"], float), np.asarray(datas[0]["cov"], float))
            opt("ba_fixed_pack", int(name.endswith("packed")))
            dev = [o["fixed_erase"][0, 0] for o in run_anchored(gpu, g, api.Params(), datas, not name.endswith("packed"))]
            opt("ba_fixed_pack", 0)
            orc = [oc.run(oracle, "anchored", d)["fixed_erase"][0, 0] for d in datas]
        elif name.startswith("pose"):
            dev = [o["outl"][0] for o in run_pose(gpu, datas)]
            orc = [oc.run(oracle, "pose", d)["outl"][0] for d in datas]
        else:
            g = api.GMM(ctx, np.asarray(datas[0]["mean"], float), np.asarray(datas[0]["cov"], float))
            dev = [o["erase"][1] for o in run_ba(gpu, g, api.Params(), datas, len(datas[0]["obs_pose"]))]
            orc = [oc.run(oracle, "ba", d)["erase"][1] for d in datas]
        kd, ko = first_flip(dev), first_flip(orc)
        out[name] = (ks[kd], ks[ko], step * (kd - ko))
        print("%s: the device's verdict flips at step %d, the oracle's at %d: chi2 distance %.1e (a quarter of the gap: %.1e)" % ((name,) + out[name] + (oc.GAP / 4,)))
    for name, (kd, ko, dist) in out.items():
        assert abs(dist) <= oc.GAP / 4, (name, kd, ko, dist)
