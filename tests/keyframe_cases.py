"""Named scenes of a few components and features on both sides of the decisions the GMM half of a key-frame makes, built by hand in
numpy, for tests/test_keyframe_cases.py (CPU: the C++ oracle and oracle/numpy_ref.py both give the output each case declares) and
tests/test_gpu_keyframe_cases.py (every case through every path of its kernel).  Test infrastructure.

The camera is hand-picked so that projections are exact: fx = fy = 512, cx = 256, cy = 192, 512 x 384, bf = 64 (mb = 0.125).  A point at
z = 1, x = -0.5 projects to u = 0 and x = +0.5 to u = 512 = width with no rounding.  Poses are the identity unless the decision needs
another.  A "plane" is a degenerate component (smallest variance 2.5e-5 or 1e-6, against the 1e-4 of is_degenerated) whose normal is
the z axis; a "blob" is not degenerate (smallest variance 1e-2).  A decision on a computed quantity has a case on either side of the
threshold at a relative distance of 1e-6: one scalar of the scene (an offset) is solved by bisection against numpy_ref, and the CPU
test re-checks the quantity on both implementations - from what they return: a chi2, the 2-D mean and covariance of a component rendered
alone, the refined point.  (A rejected triangulation returns no point: there the quantity is numpy_ref's arithmetic alone, tri_errs below,
and the oracle is held by its decision.)  Every case declares the call, the decision, its side and the integers of the
output (ids, candidates, types; for points whether they move).  The decisions and the reference lines (DECISIONS holds the same list):

  renderView (gaussian_mixture.cpp:271-371)
    view.cos          :286-301  degenerate and |po . axis0| < cos 78 deg -> dropped          cos 78 deg (1 -/+ 1e-6); a non-degenerate one at the angle
    view.behind       pinhole_camera.cpp:127-150  z > 0                                   z = 0, z < 0 projecting inside, z > 0
    view.image        pinhole_camera.cpp:127-150  0 <= u < width, 0 <= v < height          u = 0, u = width, v = 0, v = height, exactly
    view.cov2d        :311-317  both 2-D eigenvalues < 4.0 -> dropped (strict)              both below; 4 (1 -/+ 1e-6) with a small one; both exactly 4.0
    view.merge        :331-348  nearest accepted by BH distance < 0.8; nearer replaces      0.8 (1 -/+ 1e-6); farther; equal depth; equal distance; empty list
    view.merge_order  :331-348  each candidate sees the list the earlier ones left          replaced then met, one old argmin twice, a chain; in one round
                                                                                            of MG = 16 (gl_view.hip), from an older round, across the boundary
    view.sort         :362-364  depth descending; bit-equal depths keep the list order      THE PROJECT'S CHOICE: std::sort leaves equal depths unspecified
    view.cap          gmmloc_hip.h  nview counts all, view_ids holds the first view_cap    above the cap, exactly the cap
  searchCorrespondence (gaussian_mixture.cpp:484-534)
    corr.gate         :520-528  2-D MDist2 < 9.0                                           9 (1 -/+ 1e-6); Euclidean order against Mahalanobis order
    corr.knn_then_gate :506-528  the gate is applied to the k nearest, a failure spends its slot   k + 1 near, the nearest fails: ncand = k - 1
    corr.fewer_than_k :506      a view of fewer than k components                           0, 1, k - 1 components; k = 1, 5, 8
    corr.tie          nanoflann  bit-equal distances: the earlier of the depth-sorted view   two means at cx -/+ 128; the tie at the k-th place
    corr.nfeat        gmmloc_hip.h  features beyond nfeat: -1 / 0                           nfeat 0 and 1 of 3
  optimizePoint (gmmloc_opt.cpp:260-342)
    pt.chi2_proj      :330      chi2_proj > 7.815                                           7.815 (1 -/+ 1e-6): disparity against plane
    pt.chi2_str       :333      tri_check_str_chi2 and chi2_str > float(thresh * lambda2)   (1 -/+ 1e-6); the check off
    pt.solver_fail    :318      a singular 3 x 3 ends optimize(), the chi2 of that iteration stand   bf = 0, lambda2 = 0 on the axis; regular
    pt.skip           gmmloc_hip.h  comp outside 0..K-1, octave outside 0..7                 -1, K, -1, 8; solved
  checkMapAssociation (gmmloc_opt.cpp:156-258)
    cma.empty         :162-164  no candidates                                               ncand 0; all -1 (the list is not empty: fallback); octave < 0
    cma.first_min     :179-197  res and chi2_proj < min_value, in order                     a duplicate at two indices; best first / last of k = 8
    cma.neighbour     :203-228  the first neighbour strictly nearer at the refined point    nearer; bit-equal; two bit-equal; 20 neighbours, the winner
                                                                                            at 0, 15, 16, last; a switch that fails (accepted / rejected)
    cma.gate          :230-235  ll > 9.0                                                    9 (1 -/+ 1e-6)
    cma.fallback      :237-256  nearest mean, only when degenerate; moved, -1 returned      degenerate; not; fails; bit-equal distances; K = 1, 16, 17
    cma.proj_z        :169-172  lambda2 * min(1, z) ^ 2                                     depth 0.5 (scaled: chi2_str passes) and 2 (clamped: chi2_proj passes)
  optimizeTriangulationVec (localization_opt.cpp:27-204)
    tri.dedup         :143-152  an index counts once, at its first position                 in both lists; twice in one; a bit-equal twin between the two occurrences
    tri.degenerate_only :155-157  only degenerate candidates                                the best is not -> the next; none is
    tri.first_min     :182-196  err_sum < min_value, in order                               duplicates across the lists; 1, 15, 16 candidates, the last wins
    tri.chi2          :176-181  e1 > th1 or e2 > th2; 7.8 stereo, 5.991 mono                (1 -/+ 1e-6) each; u_right -0.0, 0.0, -1; oct2 ignored
    tri.chi2_str      :172-175  as pt.chi2_str                                              (1 -/+ 1e-6); the check off
    tri.skip          gmmloc_hip.h  oct1 outside 0..7                                       -1, 8; solved
  createMapPoints, per match (localization_opt.cpp:286-420)
    cmp.parallax      :311-334  cosRays < cosStereo, > 0, stereo or < 0.9998                the floats around 0.9998; 90 deg and either side; stereo on
                                                                                            side 1, 2, both; neither
    cmp.depth_vs_uright :116-137, :313  u_right >= 0 with depth <= 0                        stereo for the parallax branch; a mono edge (5.991) in the optimisation
    cmp.project       :352-368  behind, outside either image                                u = 0 and u = width in either key-frame; behind key-frame 1, 2
    cmp.reproj        :370-391  err > 7.8 s2 (stereo), 5.991 s2 (mono), s2 of key-point 1   (1 -/+ 1e-6) for each threshold in each key-frame, octave 0 and 3, oct2 another
    cmp.scale         :393-404  ratio_dist * factor < ratio_octave, ratio_dist > ratio_octave * factor   exact floats at 1.25; bisection at 1.2
    cmp.type          :407-419  0 rejected, 1 mono, 2 mono + GMM, 3 stereo, 4 stereo + GMM   each
  cmp.dist_eps (:393: a distance <= FLT_EPSILON to a camera centre) has no case: a point that near a centre and in front of it fails the
  scale test (the other distance is not small) or, with both distances small, the stereo reprojection test, whichever way that test goes.

The regime scenes (needle_fan, long_list, big_map_257, big_map_1025) are the smallest scenes on which k_search2d leaves its common
path; they declare no output by hand (it is the oracle's) but a property that shows the regime was entered."""
import numpy as np

from gmmloc_amd import api
from oracle import numpy_ref

f32, f64 = np.float32, np.float64
CAM5 = dict(fx=512.0, fy=512.0, cx=256.0, cy=192.0, bf=64.0, width=512, height=384)
ID7 = np.array([0, 0, 0, 1, 0, 0, 0], f64)
MG = 16  # gl_view.hip: candidates per merge round
REL = 1e-6

DECISIONS = {
    "view.cos": "gaussian_mixture.cpp:286-301", "view.behind": "pinhole_camera.cpp:127-150", "view.image": "pinhole_camera.cpp:127-150",
    "view.cov2d": "gaussian_mixture.cpp:311-317", "view.merge": "gaussian_mixture.cpp:331-348", "view.merge_order": "gaussian_mixture.cpp:331-348",
    "view.sort": "gaussian_mixture.cpp:362-364", "view.cap": "gmmloc_hip.h gl_search2d",
    "corr.gate": "gaussian_mixture.cpp:520-528", "corr.knn_then_gate": "gaussian_mixture.cpp:506-528", "corr.fewer_than_k": "gaussian_mixture.cpp:506",
    "corr.tie": "nanoflann.hpp:160-196", "corr.nfeat": "gmmloc_hip.h gl_search2d",
    "pt.chi2_proj": "gmmloc_opt.cpp:330", "pt.chi2_str": "gmmloc_opt.cpp:333", "pt.solver_fail": "gmmloc_opt.cpp:318", "pt.skip": "gmmloc_hip.h gl_optimize_point",
    "cma.empty": "gmmloc_opt.cpp:162-164", "cma.first_min": "gmmloc_opt.cpp:179-197", "cma.neighbour": "gmmloc_opt.cpp:203-228",
    "cma.gate": "gmmloc_opt.cpp:230-235", "cma.fallback": "gmmloc_opt.cpp:237-256", "cma.proj_z": "gmmloc_opt.cpp:169-172",
    "tri.dedup": "localization_opt.cpp:143-152", "tri.degenerate_only": "localization_opt.cpp:155-157", "tri.first_min": "localization_opt.cpp:182-196",
    "tri.chi2": "localization_opt.cpp:176-181", "tri.chi2_str": "localization_opt.cpp:172-175", "tri.skip": "gmmloc_hip.h gl_optimize_triangulation",
    "cmp.parallax": "localization_opt.cpp:311-334", "cmp.depth_vs_uright": "localization_opt.cpp:116-137", "cmp.project": "localization_opt.cpp:352-368",
    "cmp.reproj": "localization_opt.cpp:370-391", "cmp.scale": "localization_opt.cpp:393-404", "cmp.type": "localization_opt.cpp:407-419",
}


def below(x):
    return np.nextafter(x, type(x)(-np.inf))


def above(x):
    return np.nextafter(x, type(x)(np.inf))


# ---- components and maps -------------------------------------------------------------------------------------------------------------
def comp(x, y, z, sx, sy, sz, R=None):
    C = np.diag([sx * sx, sy * sy, sz * sz]).astype(f64)
    if R is not None:
        C = R @ C @ R.T
        C = 0.5 * (C + C.T)
    return (np.array([x, y, z], f64), C)


def plane(x, y, z, s=0.02, t=0.001):
    """degenerate (variance t^2 along z, far below 1e-4), facing a camera that looks along z"""
    return comp(x, y, z, s, s, t)


def blob(x, y, z, s=0.1):
    """not degenerate (every variance >= 1e-2)"""
    return comp(x, y, z, s, s, s)


def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], f64)


def mk_map(comps):
    return np.stack([c[0] for c in comps]), np.stack([c[1] for c in comps])


def camera(cam):
    return api.Camera(**cam)


# ---- one face over the C++ oracle (tests/oracle_lib.Oracle) and oracle/numpy_ref ----------------------------------------------------------
PRM_KEYS = ("tri_lambda2", "tri_str_thresh", "tri_check_str_chi2")


class Ref:
    """A map on one of the two CPU implementations, with the calls of this file under one set of names and arguments."""

    def __init__(self, backend, mean, cov, prm=None):
        self.b, self.np = backend, backend is numpy_ref
        self.mean, self.cov = np.ascontiguousarray(mean, f64), np.ascontiguousarray(cov, f64).reshape(-1, 3, 3)
        self.K = self.mean.shape[0]
        prm = prm or {}
        assert all(k in PRM_KEYS for k in prm)
        if self.np:
            self.comps = numpy_ref.build_components(self.mean, self.cov)
            self.prm = numpy_ref.Prm()
            for k, v in prm.items():
                setattr(self.prm, k, bool(v) if k == "tri_check_str_chi2" else f32(v))
            self._nbs = None
            self._view = None
        else:
            self.h = backend.gmm_create(self.mean, self.cov.reshape(-1, 9))
            self.prm = type(backend.prm).from_buffer_copy(backend.prm)
            for k, v in prm.items():
                setattr(self.prm, k, v)

    def close(self):
        if not self.np:
            self.b.gmm_destroy(self.h)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def nbs(self):
        if self._nbs is None:
            self._nbs = [r[0] for r in numpy_ref.neighbour_rows(self.mean, self.cov, self.comps["det"], range(self.K), self.prm.neighbor_dist_thresh)]
        return self._nbs

    def axis0(self, k):
        if self.np:
            return self.comps["axis"][k][:, 0]
        return self.b.gmm_get(self.h)["axis"].reshape(-1, 3, 3)[k][:, 0]

    def chi2(self, k, x):
        if self.np:
            d = np.asarray(x, f64) - self.mean[k]
            return float(d @ self.comps["cov_inv"][k] @ d)
        return float(self.b.chi2(self.h, np.array([k], np.int32), np.asarray(x, f64)[None])[0])

    def view(self, cam, pose):
        """-> ids, mean2d (V, 2), cov2d (V, 2, 2), depth"""
        if self.np:
            self._view = numpy_ref.render_view(self.mean, self.cov, self.comps, camera(cam), pose)
            v = self._view
            return (np.array([g["id"] for g in v], np.int32), np.array([g["mean"] for g in v], f64).reshape(-1, 2),
                    np.array([g["cov"] for g in v], f64).reshape(-1, 2, 2), np.array([g["depth"] for g in v], f64))
        ids, m2, c2, dep = self.b.render_view(self.h, camera(cam), pose)
        return ids, m2, c2.reshape(-1, 2, 2), dep

    def corr(self, uv, k):
        """on the last view"""
        uv = np.ascontiguousarray(uv, f64).reshape(-1, 2)
        if uv.shape[0] == 0:
            return np.zeros((0, k), np.int32), np.zeros(0, np.int32)
        if self.np:
            return numpy_ref.search_correspondence(self._view, uv, k)
        return self.b.search_correspondence(self.h, uv, k)

    def pt(self, cam, pts, uvr, octave, pose, comp_, pz2):
        if not self.np:
            return self.b.optimize_point(self.h, camera(cam), pts, uvr, octave, pose, comp_, pz2, prm=self.prm)
        r = [numpy_ref.optimize_point(pts[i], uvr[i], int(octave[i]), pose[i], self.comps["axis"][comp_[i]][:, 0], self.mean[comp_[i]], float(pz2[i]),
                                      camera(cam), self.prm) for i in range(len(pts))]
        return (np.array([x[0] for x in r], np.uint8), np.array([x[1] for x in r], f64), np.array([x[2] for x in r], f64),
                np.array([x[3] for x in r], f64).reshape(-1, 3))

    def cma(self, cam, pose, pts, uvr, octave, cand, ncand):
        if not self.np:
            return self.b.check_map_association(self.h, camera(cam), pose, pts, uvr, octave, cand, ncand, prm=self.prm)
        r = [numpy_ref.check_map_association(pts[i], uvr[i], int(octave[i]), pose, cand[i], self.comps, self.mean, self.nbs(), camera(cam), self.prm, ncand=int(ncand[i]))
             for i in range(len(pts))]
        return np.array([x[0] for x in r], np.int32), np.array([x[1] for x in r], f64).reshape(-1, 3)

    def tri(self, cam, x3d, pose1, uvr1, oct1, pose2, uvr2, oct2, cand1, n1, cand2, n2):
        if not self.np:
            return self.b.optimize_triangulation(self.h, camera(cam), x3d, pose1, uvr1, oct1, pose2, uvr2, oct2, cand1, n1, cand2, n2, prm=self.prm)
        r = [numpy_ref.optimize_triangulation(x3d[i], pose1[i], uvr1[i], int(oct1[i]), pose2[i], uvr2[i], cand1[i][:n1[i]], cand2[i][:n2[i]], self.comps,
                                              self.mean, camera(cam), self.prm) for i in range(len(x3d))]
        return np.array([x[0] for x in r], np.int32), np.array([x[1] for x in r], f64).reshape(-1, 3)

    def cmp(self, cam, pose1, uvr1, depth1, oct1, pose2, uvr2, depth2, oct2, cand1, n1, cand2, n2, scale_factor):
        if not self.np:
            return self.b.create_map_points(self.h, camera(cam), pose1, uvr1, depth1, oct1, pose2, uvr2, depth2, oct2, cand1, n1, cand2, n2,
                                            scale_factor=scale_factor, prm=self.prm)
        N = len(oct1)
        x, t, c = np.zeros((N, 3)), np.zeros(N, np.int32), np.zeros(N, np.int32)
        for i in range(N):
            p, t[i], c[i] = numpy_ref.create_map_point(pose1[i], uvr1[i], f32(depth1[i]), int(oct1[i]), pose2[i], uvr2[i], f32(depth2[i]), int(oct2[i]),
                                                       cand1[i][:n1[i]], cand2[i][:n2[i]], self.comps, self.mean, camera(cam), self.prm, scale_factor)
            if p is not None:
                x[i] = p
        return x, t, c


PT_KEYS = ("pts", "uvr", "oct", "pose", "comp", "pz2")
CMA_KEYS = ("pose", "pts", "uvr", "oct", "cand", "ncand")
TRI_KEYS = ("x3d", "pose1", "uvr1", "oct1", "pose2", "uvr2", "oct2", "cand1", "n1", "cand2", "n2")
CMP_KEYS = ("pose1", "uvr1", "depth1", "oct1", "pose2", "uvr2", "depth2", "oct2", "cand1", "n1", "cand2", "n2")


def cut_ids(ids, view_cap):
    """the view list as gl_search2d returns it: the first view_cap ids, -1 padded (no view_cap: the list itself, at least one slot)"""
    cap = view_cap or max(len(ids), 1)
    out = -np.ones(cap, np.int32)
    out[:min(cap, len(ids))] = ids[:cap]
    return out


def run(backend, call, data):
    """One call of a case on the oracle object or on numpy_ref -> dict of outputs, named and shaped as the device's.  What
    include/gmmloc_hip.h states for inputs the reference never sees (view_cap, nfeat, a component or octave outside its range) is
    applied here, since neither CPU implementation takes such inputs."""
    with Ref(backend, data["mean"], data["cov"], data.get("prm")) as r:
        cam = data["cam"]
        if call == "view":
            ids, _, _, _ = r.view(cam, data["pose"])
            uv, k = data["uv"], data["k"]
            N = uv.shape[0]
            nf = N if data.get("nfeat") is None else int(data["nfeat"])
            cand, ncand = -np.ones((N, k), np.int32), np.zeros(N, np.int32)
            cand[:nf], ncand[:nf] = r.corr(uv[:nf], k)
            return dict(ids=cut_ids(ids, data.get("view_cap")), nview=len(ids), cand=cand, ncand=ncand)
        if call == "pt":
            d = {k: data[k] for k in PT_KEYS}
            N = len(d["oct"])
            ok = (d["comp"] >= 0) & (d["comp"] < r.K) & (d["oct"] >= 0) & (d["oct"] <= 7)
            res, c2p, c2s, est = np.zeros(N, np.uint8), np.zeros(N), np.zeros(N), d["pts"].copy()
            if ok.any():
                res[ok], c2p[ok], c2s[ok], est[ok] = r.pt(cam, *[d[k][ok] for k in PT_KEYS])
            return dict(res=res, c2p=c2p, c2s=c2s, est=est)
        if call == "cma":
            d = {k: data[k] for k in CMA_KEYS}
            ok = d["oct"] >= 0
            out, pts = -np.ones(len(ok), np.int32), d["pts"].copy()
            if ok.any():
                out[ok], pts[ok] = r.cma(cam, d["pose"], d["pts"][ok], d["uvr"][ok], d["oct"][ok], d["cand"][ok], d["ncand"][ok])
            return dict(out=out, pts=pts)
        if call == "tri":
            d = {k: data[k] for k in TRI_KEYS}
            ok = (d["oct1"] >= 0) & (d["oct1"] <= 7)
            out, x = -np.ones(len(ok), np.int32), d["x3d"].copy()
            if ok.any():
                out[ok], x[ok] = r.tri(cam, *[d[k][ok] for k in TRI_KEYS])
            return dict(out=out, x=x)
        assert call == "cmp"
        x, t, c = r.cmp(cam, *[data[k] for k in CMP_KEYS], data.get("scale_factor", 1.2))
        return dict(x=x, type=t, comp=c)


class Case:
    def __init__(self, name, call, decision, side, data, want, band=None, tie=None, check=None):
        assert decision in DECISIONS, decision
        self.name, self.call, self.decision, self.side, self.data, self.want = name, call, decision, side, data, want
        self.band, self.tie, self.check = band, tie, check  # check(numpy Ref of the map, data): what the scene assumes

    def __repr__(self):
        return self.name


CASES = {}
PAIRS = []    # (case, case, output name, element): of the integer outputs the two differ in exactly that element of that output - and, where
              # that output is a count, in the list it counts (FOLLOWS), somewhere
FOLLOWS = {"nview": ("ids",), "ncand": ("cand",)}
REGIMES = {}  # name -> dict(data, prop): prop(numpy view outputs) must hold


def add(name, call, decision, side, data, want, **kw):
    assert name not in CASES, name
    CASES[name] = Case(name, call, decision, side, data, want, **kw)
    return name


def pair(a, b, out, elem=0):
    PAIRS.append((a, b, out, elem))


def solve(f, target, lo, hi):
    """x between lo and hi with f(x) = target, f monotone: bisection down to neighbouring doubles"""
    sl = f(lo) < target
    assert sl != (f(hi) < target), "the target is not between the ends"
    while True:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            return mid
        if (f(mid) < target) == sl:
            lo = mid
        else:
            hi = mid


def flip(decide, lo, hi):
    """lo, hi (one float type) on which decide differs -> the adjacent representable values (a on lo's side, b)"""
    t = type(lo)
    dl = decide(lo)
    assert dl != decide(hi), "the two ends decide alike"
    while True:
        mid = t(lo / 2 + hi / 2)
        if mid == lo or mid == hi:
            break
        if decide(mid) == dl:
            lo = mid
        else:
            hi = mid
    return lo, hi


def sides(thr):
    return (("below", thr * (1 - REL)), ("above", thr * (1 + REL)))


def in_band(q, thr, side):
    r = q / thr
    return (1 - 2e-6 <= r <= 1 - 0.5e-6) if side == "below" else (1 + 0.5e-6 <= r <= 1 + 2e-6)


def alone(backend, c, cam=CAM5, pose=ID7):
    """the 2-D component of c rendered alone -> (mean2d, cov2d, depth), or None when it is not rendered"""
    with Ref(backend, c[0][None], c[1][None]) as r:
        ids, m2, c2, dep = r.view(cam, pose)
        return (m2[0], c2[0], dep[0]) if len(ids) else None


def bh2(a, b):
    return float(numpy_ref.bh(a[0], a[1], np.linalg.det(a[1]), b[0], b[1], np.linalg.det(b[1])))


# ================================================ renderView + searchCorrespondence ====================================================
NOUV = np.zeros((0, 2), f64)


def V(name, decision, side, comps, ids, cam=CAM5, pose=ID7, uv=NOUV, k=5, cand=None, ncand=None, view_cap=None, nfeat=None, nview=None, **kw):
    mean, cov = mk_map(comps)
    uv = np.ascontiguousarray(uv, f64).reshape(-1, 2)
    data = dict(mean=mean, cov=cov, cam=cam, pose=np.array(pose, f64), uv=uv, k=k, view_cap=view_cap, nfeat=nfeat)
    want = dict(ids=np.array(ids[:view_cap] + [-1] * max(0, (view_cap or 1) - len(ids)), np.int32), nview=len(ids) if nview is None else nview)  # written out
    if cand is not None:
        want["cand"], want["ncand"] = np.array(cand, np.int32).reshape(-1, k), np.array(ncand, np.int32)
    return add(name, "view", decision, side, data, want, **kw)


ANCHOR = plane(0, 0, 4.0, s=0.08)  # u = 256, v = 192, 10 px wide: never near the component under test

# ---- view.cos: the normal tilted about y by a: |po . axis0| = cos a for a component on the optical axis
_COS78 = float(np.cos(78.0 * np.pi / 180.0))


def _tilted(a, t):
    return comp(0, 0, 2.0, 0.05, 0.05, t, rot_y(a))


def _q_cos(c):
    def q(backend):
        with Ref(backend, c[0][None], c[1][None]) as r:
            return abs(float(r.axis0(0) @ (c[0] / np.linalg.norm(c[0]))))
    return q


for _s, _t in sides(_COS78):
    _c = _tilted(float(np.arccos(_t)), 0.001)
    V("view_cos_" + _s, "view.cos", "dropped" if _s == "below" else "kept", [_c], [] if _s == "below" else [0], band=dict(thr=_COS78, side=_s, q=_q_cos(_c)))
pair("view_cos_below", "view_cos_above", "nview")
V("view_cos_nondegenerate_at_the_angle", "view.cos", "not degenerate: never tested", [_tilted(float(np.arccos(_COS78 * (1 - REL))), 0.02)], [0],
  check=lambda r, d: not r.comps["is_deg"][0] and abs(abs(float(r.axis0(0) @ [0, 0, 1.0])) / _COS78 - (1 - REL)) < 1e-9)  # (variance 4e-4; its thin axis at the angle)
V("view_cos_edge_on", "view.cos", "dropped", [_tilted(np.pi / 2, 0.001), ANCHOR], [1])

# ---- view.behind / view.image
V("view_z_zero", "view.behind", "z = 0: dropped", [plane(0.1, 0.05, 0.0), ANCHOR], [1])
V("view_z_negative_projects_inside", "view.behind", "z < 0: dropped", [plane(0.1, 0.05, -1.0), ANCHOR], [1])
V("view_z_positive", "view.behind", "z > 0: kept", [plane(0.1, 0.05, 1.0), ANCHOR], [1, 0])
pair("view_z_negative_projects_inside", "view_z_positive", "nview")
V("view_u_0", "view.image", "u = 0: kept", [plane(-0.5, 0, 1.0), ANCHOR], [1, 0])
V("view_u_width", "view.image", "u = width: dropped", [plane(0.5, 0, 1.0), ANCHOR], [1])
V("view_v_0", "view.image", "v = 0: kept", [plane(0, -0.75, 2.0), ANCHOR], [1, 0])
V("view_v_height", "view.image", "v = height: dropped", [plane(0, 0.75, 2.0), ANCHOR], [1])
V("view_u_below_0", "view.image", "u < 0: dropped", [plane(below(f64(-0.5)), 0, 1.0), ANCHOR], [1])
V("view_u_below_width", "view.image", "u < width: kept", [plane((below(f64(512.0)) - 256.0) / 512.0, 0, 1.0), ANCHOR], [1, 0])
pair("view_u_0", "view_u_below_0", "nview")
pair("view_u_width", "view_u_below_width", "nview")
# the same boundary with the principal point on the image edge: cx = 0 (the axis itself is u = 0) and cx = width
V("view_cx_0_on_axis", "view.image", "u = cx = 0: kept", [plane(0, 0, 1.0)], [0], cam=dict(CAM5, cx=0.0))
V("view_cx_width_on_axis", "view.image", "u = cx = width: dropped", [plane(0, 0, 1.0)], [], cam=dict(CAM5, cx=512.0))

# ---- view.cov2d: on the axis at z = 256 the Jacobian is 2 I: cov2d = 4 cov3d[:2, :2] exactly
def _q_eig(c_probe):
    def q(backend):
        a = alone(backend, c_probe)
        return None if a is None else float(a[1][0, 0])
    return q


V("view_cov2d_both_exactly_4", "view.cov2d", "both 4.0: kept (the test is strict)", [comp(0, 0, 256.0, 1.0, 1.0, 1.0)], [0])
V("view_cov2d_both_below", "view.cov2d", "both below: dropped", [comp(0, 0, 256.0, 0.99, 0.99, 1.0)], [])
pair("view_cov2d_both_exactly_4", "view_cov2d_both_below", "nview")
for _s, _t in sides(4.0):
    _sx = float(np.sqrt(_t / 4.0))
    # the probe has the other eigenvalue large, so that both implementations render it and show cov2d[0, 0]
    V("view_cov2d_one_" + _s, "view.cov2d", "dropped" if _s == "below" else "kept", [comp(0, 0, 256.0, _sx, 0.5, 1.0)], [] if _s == "below" else [0],
      band=dict(thr=4.0, side=_s, q=_q_eig(comp(0, 0, 256.0, _sx, 2.0, 1.0))))
pair("view_cov2d_one_below", "view_cov2d_one_above", "nview")

# ---- view.merge.  Planes of 2-D sigma 5.12 px at z = 2 (s = 0.02): BH = dx^2 / (8 sigma^2) for equal covariances.
_A = plane(0, 0, 2.0)


def _near(dx, z):
    return plane(dx, 0, z)


def _q_bh(a, b):
    return lambda backend: bh2(alone(backend, a), alone(backend, b))


for _s, _t in sides(0.8):
    _dx = solve(lambda x: bh2(alone(numpy_ref, _A), alone(numpy_ref, _near(x, 1.9))), _t, 0.0, 0.2)
    V("view_merge_bh_" + _s, "view.merge", "merged, the nearer one replaces" if _s == "below" else "kept apart", [_A, _near(_dx, 1.9)],
      [1] if _s == "below" else [0, 1], band=dict(thr=0.8, side=_s, q=_q_bh(_A, _near(_dx, 1.9))))
pair("view_merge_bh_below", "view_merge_bh_above", "nview")
V("view_merge_farther_discarded", "view.merge", "farther: discarded", [_A, _near(0.01, 2.1)], [0])
V("view_merge_nearer_replaces", "view.merge", "nearer: replaces", [_A, _near(0.01, 1.9)], [1])
V("view_merge_equal_depth_old_stays", "view.merge", "bit-equal depth: the old one stays", [_A, _near(0.01, 2.0)], [0])
pair("view_merge_nearer_replaces", "view_merge_equal_depth_old_stays", "ids")
# two accepted slots mirrored about the axis, the candidate on it: both distances bit-equal, the first slot is the argmin and is replaced
_M = [plane(-0.04, 0, 2.0), plane(0.04, 0, 2.0), plane(0, 0, 1.9)]
V("view_merge_equal_distance_first_slot", "view.merge", "bit-equal distances: the first slot", _M, [1, 2],
  tie=lambda: (bh2(alone(numpy_ref, _M[0]), alone(numpy_ref, _M[2])), bh2(alone(numpy_ref, _M[1]), alone(numpy_ref, _M[2]))))
V("view_merge_first_candidate", "view.merge", "empty list: appended", [_A], [0])

# ---- view.merge_order: fillers on a 64 px grid at z = 2 (BH about 19 between neighbours), the interacting three in the bottom row:
# S at x = 0, P at +0.04 (BH(S, P) about 0.5), Q at +0.08 (BH(S, Q) about 2, BH(P, Q) about 0.5) or at -0.04 (BH(P, Q) about 2)
def _filler(i):
    return plane(-0.875 + 0.25 * (i % 8), -0.625 + 0.25 * (i // 8), 2.0)


def _ordered(at, trio):
    """the three comps of trio at indices `at` of a map otherwise made of fillers -> comps"""
    n, out, j = max(at) + 1, [], 0
    for i in range(n):
        if i in at:
            out.append(trio[at.index(i)])
        else:
            out.append(_filler(j))
            j += 1
    return out


def _S(z=1.99):
    return plane(0, 0.625 * z / 2.0, z)


def _P(x, z):
    return plane(x * z / 2.0, 0.625 * z / 2.0, z)


for _n, _at in (("one_round", (13, 14, 15)), ("old_slot", (0, 16, 17)), ("across_rounds", (15, 16, 17))):
    _fill = [i for i in range(max(_at) + 1) if i not in _at]
    # S <- P (nearer) <- Q (nearer than P, near P only): one slot, holding Q
    V("view_order_chain_" + _n, "view.merge_order", "replaced, then met by the next: a chain", _ordered(_at, [_S(), _P(0.04, 1.98), _P(0.08, 1.97)]), _fill + [_at[2]])
    # ... Q farther than P: it meets P, not S, and is discarded
    V("view_order_met_and_discarded_" + _n, "view.merge_order", "replaced, then met by a farther one", _ordered(_at, [_S(), _P(0.04, 1.98), _P(0.08, 1.985)]),
      _fill + [_at[1]])
    # P and Q both have S as their nearest old slot; after P took it, Q is far from what the slot holds and is appended
    V("view_order_same_argmin_" + _n, "view.merge_order", "two candidates with one old argmin", _ordered(_at, [_S(), _P(0.04, 1.98), _P(-0.04, 1.97)]),
      _fill + [_at[1], _at[2]])
pair("view_order_chain_across_rounds", "view_order_met_and_discarded_across_rounds", "ids", 15)

# ---- view.sort
V("view_sort_descending", "view.sort", "depth descending", [plane(-0.25, 0, 1.0), plane(0, 0, 2.0), plane(0.75, 0, 3.0)], [2, 1, 0])
# A (index 0) is replaced by B (index 2) in slot 0; F (index 1) has B's depth bit for bit: the list order [B, F] stays
V("view_sort_equal_depth_list_order", "view.sort", "bit-equal depths: the list order (the project's choice), not the index",
  [plane(-0.5, 0, 2.0), plane(0.475, 0, 1.9), plane(-0.5 * 1.9 / 2.0 + 0.01, 0, 1.9)], [2, 1])
V("view_sort_equal_depth_index_order", "view.sort", "bit-equal depths: the list order, here the index order",
  [plane(-0.5, 0, 1.9), plane(0.475, 0, 1.9), plane(0.0, 0, 2.0)], [2, 0, 1])

# ---- view.cap
_FIVE = [plane(-0.75 + 0.375 * i, 0, 2.0 + 0.1 * i) for i in range(5)]
# (the feature sits on component 0, the last of the view and beyond the cap: the tables are searched over the whole view)
V("view_cap_above", "view.cap", "more than view_cap: nview counts all", _FIVE, [4, 3, 2, 1, 0], view_cap=3, nview=5, uv=[[64.0, 192.0]], cand=[[0, -1, -1, -1, -1]], ncand=[1])
V("view_cap_exact", "view.cap", "exactly view_cap", _FIVE, [4, 3, 2, 1, 0], view_cap=5)
V("view_cap_below", "view.cap", "fewer than view_cap: -1 padded", _FIVE, [4, 3, 2, 1, 0], view_cap=7)

# ---- corr.gate
_G = plane(0, 0, 1.0)  # 2-D sigma 10.24 px
for _s, _t in sides(9.0):
    _d = solve(lambda d: d * d / alone(numpy_ref, _G)[1][0, 0], _t, 1.0, 100.0)

    def _q(backend, _d=_d):
        m2, c2, _ = alone(backend, _G)
        e = np.array([256.0 + _d, 192.0]) - m2
        return float(e @ np.linalg.inv(c2) @ e)
    V("corr_gate_" + _s, "corr.gate", "taken" if _s == "below" else "not taken", [_G], [0], uv=[[256.0 + _d, 192.0]], cand=[[0, -1, -1, -1, -1] if _s == "below" else [-1] * 5],
      ncand=[1 if _s == "below" else 0], band=dict(thr=9.0, side=_s, q=_q))
pair("corr_gate_below", "corr_gate_above", "ncand")
# A (index 0): 51.2 x 5.12 px at (256, 192); B (index 1): 5.12 px at (296, 212); C (index 2): 51.2 px at (396, 192).  The feature (296, 192) is
# 20 px from B (MDist2 15.3: fails), 40 px from A (0.6), 100 px from C (3.8)
_ANI = [comp(0, 0, 1.0, 0.1, 0.01, 0.001), plane(40 / 512, 20 / 512, 1.0, s=0.01), plane(140 / 512, 0, 1.0, s=0.1)]
V("corr_euclidean_order_k1", "corr.gate", "the Euclidean nearest fails the gate: nothing, though the Mahalanobis nearest would pass", _ANI[:2], [0, 1],
  uv=[[296.0, 192.0]], k=1, cand=[[-1]], ncand=[0])
V("corr_euclidean_order_k2", "corr.gate", "the second Euclidean nearest passes", _ANI[:2], [0, 1], uv=[[296.0, 192.0]], k=2, cand=[[0, -1]], ncand=[1])
V("corr_knn_then_gate_k2", "corr.knn_then_gate", "k + 1 near, the nearest fails: ncand = k - 1, the (k + 1)-th not taken", _ANI, [0, 1, 2], uv=[[296.0, 192.0]], k=2,
  cand=[[0, -1]], ncand=[1])
V("corr_knn_then_gate_k3", "corr.knn_then_gate", "k = 3 reaches the third", _ANI, [0, 1, 2], uv=[[296.0, 192.0]], k=3, cand=[[0, 2, -1]], ncand=[2])
pair("corr_knn_then_gate_k2", "corr_euclidean_order_k2", "nview")

# ---- corr.fewer_than_k: components of 51.2 px at z = 2 on a hexagon of radius 140 px round the image centre and one in it
def _hex(n):
    pts = [(0.0, 0.0)] + [(140 * np.cos(np.pi * i / 3 + 0.3), 140 * np.sin(np.pi * i / 3 + 0.3)) for i in range(6)]
    return [plane(p[0] / 256, p[1] / 256, 2.0, s=0.2) for p in pts[:n]], np.array(pts[:n]) + [256.0, 192.0]


_FEAT = np.array([[259.0, 193.7]])
for _n, _k in ((1, 5), (4, 5), (7, 8), (1, 1), (5, 5)):
    _c, _m = _hex(_n)
    _o = np.argsort(((_FEAT - _m) ** 2).sum(1))[:_k]  # distinct distances: (3, 1.7) off the centre
    V("corr_view_of_%d_k%d" % (_n, _k), "corr.fewer_than_k", "%d of k = %d" % (_n, _k) if _n < _k else "k of k", _c, list(range(_n)), uv=_FEAT, k=_k,
      cand=[list(_o) + [-1] * (_k - len(_o))], ncand=[len(_o)])
V("corr_view_of_0_k5", "corr.fewer_than_k", "an empty view", [plane(0, 0, -1.0)], [], uv=_FEAT, k=5, cand=[[-1] * 5], ncand=[0])

# ---- corr.tie: index 0 at u = 128 (z = 1), index 1 at u = 384 (z = 2): the view is [1, 0]; the feature at u = 256 is 128 px from both
_TIE = [plane(-0.25, 0, 1.0, s=0.1), plane(0.5, 0, 2.0, s=0.2), plane(0, 0.125, 1.0, s=0.05)]
_UV0 = np.array([[256.0, 192.0]])


def _tie_d2():
    _, m2, _, _ = Ref(numpy_ref, *mk_map(_TIE[:2])).view(CAM5, ID7)
    d = ((_UV0 - m2) ** 2).sum(1)
    return d[0], d[1]


V("corr_tie_k2", "corr.tie", "bit-equal distances: the order of the view", _TIE[:2], [1, 0], uv=_UV0, k=2, cand=[[1, 0]], ncand=[2], tie=_tie_d2)
V("corr_tie_k1", "corr.tie", "the tie decides who is in", _TIE[:2], [1, 0], uv=_UV0, k=1, cand=[[1]], ncand=[1], tie=_tie_d2)
def _tie3_d2():
    _, m2, _, _ = Ref(numpy_ref, *mk_map(_TIE)).view(CAM5, ID7)  # the view is [1, 0, 2]
    d = ((_UV0 - m2) ** 2).sum(1)
    assert d[2] < d[0]
    return d[0], d[1]


V("corr_tie_at_kth", "corr.tie", "the tie at the k-th place", _TIE, [1, 0, 2], uv=_UV0, k=2, cand=[[2, 1]], ncand=[2], tie=_tie3_d2)
V("corr_no_tie_k2", "corr.tie", "no tie: the nearer first", _TIE[:2], [1, 0], uv=[[255.0, 192.0]], k=2, cand=[[0, 1]], ncand=[2])
_UV3 = np.array([[256.0, 192.0], [130.0, 192.0], [380.0, 190.0]])
V("corr_nfeat_all", "corr.nfeat", "nfeat = N", _TIE[:2], [1, 0], uv=_UV3, k=2, cand=[[1, 0], [0, -1], [1, -1]], ncand=[2, 1, 1])
V("corr_nfeat_1", "corr.nfeat", "nfeat 1 of 3", _TIE[:2], [1, 0], uv=_UV3, k=2, nfeat=1, cand=[[1, 0], [-1, -1], [-1, -1]], ncand=[2, 0, 0])
V("corr_nfeat_0", "corr.nfeat", "nfeat 0 of 3", _TIE[:2], [1, 0], uv=_UV3, k=2, nfeat=0, cand=[[-1, -1]] * 3, ncand=[0, 0, 0])

# ================================================ optimizePoint ==========================================================================
# A feature on the optical axis: u, v do not depend on its depth, u_right = 256 - 64 / z does.  A plane z = zp disagrees with the stereo depth
# z0 by d = zp - z0: chi2_proj and chi2_str grow with |d|, smoothly (the in-plane directions carry no error).
def PL(zp, x=0.0, y=0.0):
    return plane(x, y, zp, s=0.05, t=0.005)


def axis_feature(z0):
    return np.array([0.0, 0.0, z0]), np.array([256.0, 192.0, 256.0 - 64.0 / z0])


def pt_data(comps, z0, ci=0, oct=0, pz2=1.0, prm=None, cam=CAM5, uvr=None, pt=None):
    mean, cov = mk_map(comps)
    p, u = axis_feature(z0)
    return dict(mean=mean, cov=cov, cam=cam, prm=prm or {}, pts=(p if pt is None else np.array(pt, f64))[None].copy(),
                uvr=(u if uvr is None else np.array(uvr, f64))[None].copy(), oct=np.array([oct], np.int32), pose=ID7[None].copy(),
                comp=np.array([ci], np.int32), pz2=np.array([pz2], f64))


def _pt_q(data, what):
    return lambda backend: float(run(backend, "pt", data)[what][0])


def PT(name, decision, side, data, res, moved, **kw):
    return add(name, "pt", decision, side, data, dict(res=np.array([res], np.uint8), moved=np.array([moved])), **kw)


STR_THR = float(f32(f32(0.0064) * f32(400.0)))
for _s, _t in sides(7.815):  # at z0 = 4 the disparity is weak against the plane: chi2_str stays near 0.04 chi2_proj
    _d = solve(lambda d: run(numpy_ref, "pt", pt_data([PL(4.0 + d)], 4.0))["c2p"][0], _t, 0.1, 1.5)
    _dat = pt_data([PL(4.0 + _d)], 4.0)
    PT("pt_chi2_proj_" + _s, "pt.chi2_proj", "res 1" if _s == "below" else "res 0", _dat, _s == "below", True, band=dict(thr=7.815, side=_s, q=_pt_q(_dat, "c2p")))
pair("pt_chi2_proj_below", "pt_chi2_proj_above", "res")
for _s, _t in sides(STR_THR):  # at z0 = 1 the disparity is stiff: chi2_str is about 5 chi2_proj
    _d = solve(lambda d: run(numpy_ref, "pt", pt_data([PL(1.0 + d)], 1.0))["c2s"][0], _t, 0.02, 0.2)
    _dat = pt_data([PL(1.0 + _d)], 1.0)
    PT("pt_chi2_str_" + _s, "pt.chi2_str", "res 1" if _s == "below" else "res 0", _dat, _s == "below", True, band=dict(thr=STR_THR, side=_s, q=_pt_q(_dat, "c2s")))
    if _s == "above":
        PT("pt_chi2_str_above_check_off", "pt.chi2_str", "the check off: res 1", pt_data([PL(1.0 + _d)], 1.0, prm=dict(tri_check_str_chi2=0)), True, True)
pair("pt_chi2_str_below", "pt_chi2_str_above", "res")
# bf = 0 and lambda2 = 0 on the axis: the third column of the Jacobian is zero, H = diag(2 s f^2 / z^2, s f^2 / z^2, 0): a zero pivot in the
# first iteration.  The errors (1, 1, 1) of that iteration stand (chi2_proj = 3), the point stays.
_SF = pt_data([PL(2.0)], 2.0, prm=dict(tri_lambda2=0.0), cam=dict(CAM5, bf=0.0), uvr=[257.0, 193.0, 257.0])
PT("pt_solver_fail", "pt.solver_fail", "singular: stops, chi2 of that iteration", _SF, True, False)
CASES["pt_solver_fail"].want.update(c2p=np.array([3.0]), c2s=np.array([0.0]))
PT("pt_solver_regular", "pt.solver_fail", "regular: iterates", pt_data([PL(2.0)], 2.0, cam=dict(CAM5, bf=0.0), uvr=[257.0, 193.0, 257.0]), True, True)
_SK = [PL(2.01), PL(2.02)]
for _n, _ci, _o in (("comp_minus_1", -1, 0), ("comp_K", 2, 0), ("octave_minus_1", 0, -1), ("octave_8", 0, 8)):
    PT("pt_skip_" + _n, "pt.skip", "not solved", pt_data(_SK, 2.0, ci=_ci, oct=_o), False, False)
    CASES["pt_skip_" + _n].want.update(c2p=np.array([0.0]), c2s=np.array([0.0]))
for _n, _ci, _o in (("comp_last", 1, 0), ("octave_7", 0, 7)):
    PT("pt_solved_" + _n, "pt.skip", "solved", pt_data(_SK, 2.0, ci=_ci, oct=_o), True, True)

# ================================================ checkMapAssociation ====================================================================
# z0 = 2, lambda2 = 400: the refined point goes about 0.76 d towards a plane d away; its chi2 to that plane is about (0.24 d / 0.005)^2.
def cma_data(comps, cands, z0=2.0, k=None, ncand=None, oct=0, prm=None):
    mean, cov = mk_map(comps)
    p, u = axis_feature(z0)
    k = k or max(len(cands), 1)
    c = -np.ones((1, k), np.int32)
    c[0, :len(cands)] = cands
    return dict(mean=mean, cov=cov, cam=CAM5, prm=prm or {}, pose=ID7.copy(), pts=p[None].copy(), uvr=u[None].copy(), oct=np.array([oct], np.int32),
                cand=c, ncand=np.array([len(cands) if ncand is None else ncand], np.int32))


def CMA(name, decision, side, data, out, moved, z_side=0, **kw):
    want = dict(out=np.array([out], np.int32), moved=np.array([moved]))
    if z_side:
        want["z_side"] = z_side  # the point ends above (+1) / below (-1) its initial depth
    return add(name, "cma", decision, side, data, want, **kw)


FAR_FAIL = PL(2.5)   # a candidate whose refinement fails both tests
_FILL3 = [PL(6.0 + i, x=1.0) for i in range(17)]  # far from everything
CMA("cma_ncand_0", "cma.empty", "ncand 0", cma_data([PL(2.001)], [], k=5), -1, False)
CMA("cma_one_candidate", "cma.empty", "a candidate", cma_data([PL(2.001)], [0], k=5), 0, True)
pair("cma_ncand_0", "cma_one_candidate", "out")
CMA("cma_all_minus_1", "cma.empty", "every candidate -1: the list is not empty, the fallback runs", cma_data([PL(2.001)], [], k=5, ncand=5), -1, True)
CMA("cma_octave_negative", "cma.empty", "octave < 0: skipped", cma_data([PL(2.001)], [0], k=5, oct=-1), -1, False)
# duplicates: index 0 and 1 are one component
CMA("cma_duplicate_higher_index_first", "cma.first_min", "bit-equal chi2: the lower position, here the higher index", cma_data([PL(2.004), PL(2.004)], [1, 0]), 1, True)
CMA("cma_duplicate_lower_index_first", "cma.first_min", "bit-equal chi2: the lower position, here the lower index", cma_data([PL(2.004), PL(2.004)], [0, 1]), 0, True)
pair("cma_duplicate_higher_index_first", "cma_duplicate_lower_index_first", "out")
_STACK = [PL(2.001)] + [PL(2.0 + 0.03 * (j + 1)) for j in range(7)]  # 0.03 apart: not neighbours (BH 4.5)
CMA("cma_best_first_of_8", "cma.first_min", "the best at position 0 of k = 8", cma_data(_STACK, [0, 1, 2, 3, 4, 5, 6, 7]), 0, True)
CMA("cma_best_last_of_8", "cma.first_min", "the best at position k - 1 of k = 8", cma_data(_STACK, [7, 6, 5, 4, 3, 2, 1, 0]), 0, True)
# neighbours: the candidate C = plane 2.012 (refined point near 2.0091), N = plane 2.009 is nearer there
CMA("cma_neighbour_nearer", "cma.neighbour", "a neighbour strictly nearer: switch", cma_data([PL(2.012), PL(2.009)], [0]), 1, True,
    check=lambda r, d: 1 in r.nbs()[0])
CMA("cma_neighbour_farther", "cma.neighbour", "a neighbour farther: no switch", cma_data([PL(2.012), PL(2.018)], [0]), 0, True, check=lambda r, d: 1 in r.nbs()[0])
pair("cma_neighbour_nearer", "cma_neighbour_farther", "out")
CMA("cma_neighbour_bit_equal", "cma.neighbour", "a duplicate neighbour, bit-equal: no switch", cma_data([PL(2.012), PL(2.012)], [1]), 1, True,
    check=lambda r, d: 0 in r.nbs()[1])
CMA("cma_two_neighbours_bit_equal", "cma.neighbour", "two bit-equal neighbours: the first of the list", cma_data([PL(2.012), PL(2.02), PL(2.009), PL(2.009)], [0]), 2, True,
    check=lambda r, d: list(r.nbs()[0]) == [1, 2, 3])
for _p in (0, 15, 16, 19):
    _c = [PL(2.012)] + [PL(2.012 + 0.0005 * (j + 1)) for j in range(20)]
    _c[1 + _p] = PL(2.009)
    CMA("cma_20_neighbours_winner_at_%d" % _p, "cma.neighbour", "a list longer than a row, the winner at %d" % _p, cma_data(_c, [0]), 1 + _p, True,
        check=lambda r, d: list(r.nbs()[0]) == list(range(1, 21)))
# a switch whose re-optimisation fails: N is a blob (normal x) whose mean is 0.1 off the axis: chi2 about 1 at the refined point, but its
# plane x = 0.1 costs chi2_str = 4 > 2.56
def _refined(d, k):
    return run(numpy_ref, "pt", dict(d, pts=d["pts"], pose=d["pose"][None], comp=np.array([k], np.int32), pz2=np.array([1.0])))


def _switch_fails(lo, hi):
    def check(r, d):
        x, n = _refined(d, 0)["est"][0], _refined(d, 1)
        return 1 in r.nbs()[0] and r.chi2(1, x) < r.chi2(0, x) and lo < r.chi2(0, x) < hi and not n["res"][0]
    return check


CMA("cma_switch_fails_back_to_candidate", "cma.neighbour", "the switch fails: back to the candidate", cma_data([PL(2.03125), comp(0.1, 0, 2.0239, 0.1, 0.2, 0.2)], [0]), 0, True,
    check=_switch_fails(1.5, 9.0))
CMA("cma_switch_fails_own_chi2_rejects", "cma.neighbour", "the switch fails: the candidate's own chi2 (above 9) decides",
    cma_data([PL(2.0667), comp(0.1, 0, 2.0511, 0.1, 0.2, 0.2)], [0]), -1, False, check=_switch_fails(9.0, 20.0))
for _s, _t in sides(9.0):
    def _ll(d):
        dat = pt_data([PL(2.0 + d)], 2.0)
        with Ref(numpy_ref, dat["mean"], dat["cov"]) as r:
            return r.chi2(0, run(numpy_ref, "pt", dat)["est"][0])
    _d = solve(_ll, _t, 0.01, 0.3)

    def _q(backend, _d=_d):
        dat = pt_data([PL(2.0 + _d)], 2.0)
        with Ref(backend, dat["mean"], dat["cov"]) as r:
            return r.chi2(0, run(backend, "pt", dat)["est"][0])
    CMA("cma_gate_" + _s, "cma.gate", "accepted" if _s == "below" else "rejected: -1, untouched", cma_data([PL(2.0 + _d)], [0]), 0 if _s == "below" else -1, _s == "below",
        band=dict(thr=9.0, side=_s, q=_q))
pair("cma_gate_below", "cma_gate_above", "out")
# fallback: the only candidate fails; queryPoint's nearest mean is tried when it is degenerate
CMA("cma_fallback_degenerate_moves", "cma.fallback", "nearest mean degenerate: moved, -1", cma_data([FAR_FAIL, PL(2.002)], [0]), -1, True, z_side=+1)
CMA("cma_fallback_not_degenerate", "cma.fallback", "nearest mean not degenerate: untouched", cma_data([FAR_FAIL, comp(0, 0, 2.01, 0.3, 0.3, 0.1), PL(2.1)], [0]), -1, False,
    check=lambda r, d: _refined(d, 1)["res"][0] and (_refined(d, 1)["est"] != d["pts"]).any())  # it would move the point were it tried
CMA("cma_fallback_fails", "cma.fallback", "nearest mean degenerate, its refinement fails: untouched", cma_data([FAR_FAIL, PL(2.4)], [0]), -1, False)
CMA("cma_fallback_K1", "cma.fallback", "K = 1: the candidate again, fails again", cma_data([FAR_FAIL], [0]), -1, False)


def _tie_map(K, up, down, cand_at):
    c = list(_FILL3[:K])
    c[up], c[down], c[cand_at] = PL(2.125), PL(1.875), FAR_FAIL
    return c


for _K, _up, _dn, _zs in ((16, 0, 15, +1), (16, 15, 0, -1), (17, 15, 16, +1), (17, 16, 15, -1), (17, 16, 0, -1), (17, 0, 16, +1)):
    CMA("cma_fallback_tie_K%d_up%d_down%d" % (_K, _up, _dn), "cma.fallback", "two means at bit-equal distance: the lowest index (K = %d)" % _K,
        cma_data(_tie_map(_K, _up, _dn, 5), [5]), -1, True, z_side=_zs,
        tie=lambda: (float(((np.array([0, 0, 2.125]) - [0, 0, 2.0]) ** 2).sum()), float(((np.array([0, 0, 1.875]) - [0, 0, 2.0]) ** 2).sum())))
# proj_z: blobs (thick along z, so that the gate passes), alone in the map.  Depth 0.5: lambda2 = 100 and chi2_str = 100 * 0.12^2 passes where 400 *
# 0.12^2 would not.  Depth 2: lambda2 stays 400 and chi2_proj stays at 7.4, where 1600 would hold the point off the disparity: above 7.815.
_BZ = lambda z: comp(0, 0, z, 0.3, 0.3, 0.1)


def _with_pz2(z0, d, pz2):
    return run(numpy_ref, "pt", pt_data([_BZ(z0 + d)], z0, pz2=pz2))


_D2 = solve(lambda d: _with_pz2(2.0, d, 1.0)["c2p"][0], 7.4, 0.1, 0.6)
CMA("cma_proj_z_half", "cma.proj_z", "depth 0.5: lambda2 scaled by 0.25", cma_data([_BZ(0.62)], [0], z0=0.5), 0, True,
    check=lambda r, d: _with_pz2(0.5, 0.12, 0.25)["res"][0] and not _with_pz2(0.5, 0.12, 1.0)["res"][0])
CMA("cma_proj_z_two", "cma.proj_z", "depth 2: clamped to 1", cma_data([_BZ(2.0 + _D2)], [0], z0=2.0), 0, True,
    check=lambda r, d: _with_pz2(2.0, _D2, 1.0)["res"][0] and not _with_pz2(2.0, _D2, 4.0)["res"][0])

# ================================================ optimizeTriangulationVec ================================================================
def two_views(P, c2, ur1=True, ur2=True, dv1=0.0, dv2=0.0):
    """key-frame 1 at the origin, key-frame 2 centred at c2, both looking along z; the point P seen by both -> pose1, uvr1, pose2, uvr2"""
    P, c2 = np.array(P, f64), np.array(c2, f64)
    q = P - c2
    u1, u2 = 512.0 * P[0] / P[2] + 256.0, 512.0 * q[0] / q[2] + 256.0
    uvr1 = np.array([u1, 512.0 * P[1] / P[2] + 192.0 + dv1, u1 - 64.0 / P[2] if ur1 else -1.0])
    uvr2 = np.array([u2, 512.0 * q[1] / q[2] + 192.0 + dv2, u2 - 64.0 / q[2] if ur2 else -1.0])
    return ID7.copy(), uvr1, np.concatenate([[0, 0, 0, 1], -c2]), uvr2


def tri_data(comps, P, c2, cand1, cand2, k=None, oct1=0, oct2=0, prm=None, uvr1=None, uvr2=None, **kw):
    mean, cov = mk_map(comps)
    p1, u1, p2, u2 = two_views(P, c2, **kw)
    k = k or max(len(cand1), len(cand2), 1)
    c1, c2_ = -np.ones((1, k), np.int32), -np.ones((1, k), np.int32)
    c1[0, :len(cand1)], c2_[0, :len(cand2)] = cand1, cand2
    return dict(mean=mean, cov=cov, cam=CAM5, prm=prm or {}, x3d=(np.array(P, f64) + [0.004, -0.003, 0.005])[None].copy(), pose1=p1[None], uvr1=(u1 if uvr1 is None else np.array(uvr1, f64))[None],
                oct1=np.array([oct1], np.int32), pose2=p2[None], uvr2=(u2 if uvr2 is None else np.array(uvr2, f64))[None], oct2=np.array([oct2], np.int32),
                cand1=c1, n1=np.array([len(cand1)], np.int32), cand2=c2_, n2=np.array([len(cand2)], np.int32))


def TRI(name, decision, side, data, out, **kw):
    return add(name, "tri", decision, side, data, dict(out=np.array([out], np.int32), moved=np.array([out >= 0])), **kw)


P2, C21 = (0.0, 0.0, 2.0), (0.5, 0.0, 1.0)   # the point 2 in front of key-frame 1 and 1 in front of key-frame 2
# 0 A: the plane through the point; 1: a blob there; 2: A again; 3 B: a plane 0.02 off; 4..18: planes 0.03 .. 0.17 off (worse and worse)
TRI_MAP = [PL(2.0), blob(0, 0, 2.0), PL(2.0), PL(2.02)] + [PL(2.03 + 0.01 * j) for j in range(15)]
_LOSERS = list(range(4, 19))
TRI("tri_same_index_in_both_lists", "tri.dedup", "the same index in cand1 and cand2", tri_data(TRI_MAP, P2, C21, [3, 0], [0, 3]), 0)
TRI("tri_index_twice_in_cand1", "tri.dedup", "twice within cand1", tri_data(TRI_MAP, P2, C21, [3, 3, 0], [0]), 0)
# 2 is 0 again (bit-equal sums): the winner is the one whose FIRST occurrence comes first; a de-duplication that kept the last would turn both round
TRI("tri_first_occurrence_counts_across_lists", "tri.dedup", "0 again in cand2, after its twin: its first position counts", tri_data(TRI_MAP, P2, C21, [0, 2], [0]), 0)
TRI("tri_first_occurrence_counts_in_cand1", "tri.dedup", "2 again in cand1, after its twin: its first position counts", tri_data(TRI_MAP, P2, C21, [2, 0, 2], []), 2)
pair("tri_first_occurrence_counts_across_lists", "tri_first_occurrence_counts_in_cand1", "out")
TRI("tri_best_not_degenerate", "tri.degenerate_only", "the best candidate is not degenerate: the next", tri_data(TRI_MAP, P2, C21, [1, 3], []), 3)
TRI("tri_none_degenerate", "tri.degenerate_only", "no candidate degenerate: -1, untouched", tri_data(TRI_MAP, P2, C21, [1], [1]), -1)
TRI("tri_degenerate", "tri.degenerate_only", "degenerate: taken", tri_data(TRI_MAP, P2, C21, [0], [1]), 0)
pair("tri_none_degenerate", "tri_degenerate", "out")
TRI("tri_duplicate_across_lists_higher_first", "tri.first_min", "bit-equal sums across the lists: the lower position (the higher index)", tri_data(TRI_MAP, P2, C21, [2], [0]), 2)
TRI("tri_duplicate_across_lists_lower_first", "tri.first_min", "bit-equal sums across the lists: the lower position (the lower index)", tri_data(TRI_MAP, P2, C21, [0], [2]), 0)
pair("tri_duplicate_across_lists_higher_first", "tri_duplicate_across_lists_lower_first", "out")
TRI("tri_1_candidate", "tri.first_min", "n1 + n2 = 1", tri_data(TRI_MAP, P2, C21, [0], [], k=8), 0)
TRI("tri_15_candidates_last_wins", "tri.first_min", "n1 + n2 = 15, the winner in the last lane", tri_data(TRI_MAP, P2, C21, _LOSERS[:8], _LOSERS[8:14] + [0], k=8), 0)
TRI("tri_16_candidates_last_wins", "tri.first_min", "n1 + n2 = 16, the winner in the last lane", tri_data(TRI_MAP, P2, C21, _LOSERS[:8], _LOSERS[8:15] + [0], k=8), 0)
TRI("tri_16_candidates_first_wins", "tri.first_min", "n1 + n2 = 16, the winner in the first lane", tri_data(TRI_MAP, P2, C21, [0] + _LOSERS[:7], _LOSERS[7:15], k=8), 0)


def tri_errs(data):
    """(e1, e2, es) of the first candidate of a case at numpy_ref's answer, or, where that answer is a rejection, at the point a copy of its
    loop reaches: the reference's errors are those before the 20th update, which differs from the point after it far below 1e-8"""
    r = Ref(numpy_ref, data["mean"], data["cov"], data.get("prm"))
    cam, prm, k = camera(data["cam"]), r.prm, int(data["cand1"][0, 0])
    n, mu = r.comps["axis"][k][:, 0], r.mean[k]
    T = [numpy_ref.SE3.from7(data["pose1"][0]), numpy_ref.SE3.from7(data["pose2"][0])]
    U = [data["uvr1"][0], data["uvr2"][0]]
    st = [not (u[2] < 0) for u in U]
    s, lam = float(prm.sigma2_inv[data["oct1"][0]]), float(prm.tri_lambda2)
    x = data["x3d"][0].copy()
    for _ in range(20):
        H, b, e = lam * np.outer(n, n), -lam * n * (n @ (x - mu)), []
        for Ti, u, sti in zip(T, U, st):
            pc, d = Ti.map(x), 3 if sti else 2
            ei = u[:d] - numpy_ref.proj_stereo(pc, cam)[:d]
            J = -numpy_ref.dproj(pc, cam, sti) @ Ti.R
            H, b = H + s * J.T @ J, b - s * J.T @ ei
            e.append(s * ei @ ei)
        es = lam * (n @ (x - mu)) ** 2
        x = x + np.linalg.solve(H, b)
    return e[0], e[1], es


def errs_at(data, x):
    """(e1, e2, es) of the first candidate at the point x an implementation returned"""
    d = dict(data, x3d=np.array(x, f64)[None])
    r = Ref(numpy_ref, data["mean"], data["cov"], data.get("prm"))
    cam, k = camera(data["cam"]), int(data["cand1"][0, 0])
    n, mu = r.comps["axis"][k][:, 0], r.mean[k]
    s, lam = float(r.prm.sigma2_inv[data["oct1"][0]]), float(r.prm.tri_lambda2)
    e = []
    for p, u in ((d["pose1"][0], d["uvr1"][0]), (d["pose2"][0], d["uvr2"][0])):
        T, dd = numpy_ref.SE3.from7(p), 2 if u[2] < 0 else 3
        ei = u[:dd] - numpy_ref.proj_stereo(T.map(d["x3d"][0]), cam)[:dd]
        e.append(s * ei @ ei)
    return e[0], e[1], lam * (n @ (d["x3d"][0] - mu)) ** 2


def _tri_q(data, i):
    def q(backend):
        o = run(backend, "tri", data)
        if o["out"][0] < 0:  # rejected: no point comes back; only this file's copy of the loop can say
            return tri_errs(data)[i] if backend is numpy_ref else None
        return errs_at(data, o["x"][0])[i]
    return q


# the offset key-frame sees the point from twice as far as the other: its residual is 0.8 of the offset, the other's 0.4
P1, C12 = (0.0, 0.0, 1.0), (0.5, 0.0, -1.0)  # 1 in front of key-frame 1, 2 in front of key-frame 2
TRI_MAP1 = [PL(1.0)]
for _e, _st, _thr in ((1, False, 5.991), (1, True, 7.8), (2, False, 5.991), (2, True, 7.8)):
    for _s, _t in sides(_thr):
        _mk = (lambda dv, _e=_e, _st=_st: tri_data(TRI_MAP, P2, C21, [0], [], ur1=_st, ur2=True, dv1=dv) if _e == 1 else
               tri_data(TRI_MAP1, P1, C12, [0], [], ur1=True, ur2=_st, dv2=dv))
        _dv = solve(lambda dv: tri_errs(_mk(dv))[_e - 1], _t, 0.5, 6.0)
        _dat = _mk(_dv)
        TRI("tri_e%d_%s_%s" % (_e, "stereo" if _st else "mono", _s), "tri.chi2", ("e%d within " if _s == "below" else "e%d above ") % _e + str(_thr), _dat,
            0 if _s == "below" else -1, band=dict(thr=_thr, side=_s, q=_tri_q(_dat, _e - 1)))
    pair("tri_e%d_%s_below" % (_e, "stereo" if _st else "mono"), "tri_e%d_%s_above" % (_e, "stereo" if _st else "mono"), "out")
TRI("tri_oct2_ignored", "tri.chi2", "oct2 = 5: both edges weighed with octave 1's sigma, same result",
    dict(CASES["tri_e2_mono_below"].data, oct2=np.array([5], np.int32)), 0)
TRI("tri_oct2_ignored_above", "tri.chi2", "oct2 = 5 would lower e2 below the threshold: still rejected", dict(CASES["tri_e2_mono_above"].data, oct2=np.array([5], np.int32)), -1)
TRI("tri_oct1_weighs_both", "tri.chi2", "oct1 = 1 lowers both errors: accepted", dict(CASES["tri_e2_mono_above"].data, oct1=np.array([1], np.int32)), 0)
# u_right = 0 exactly: the point (-0.125, 0, 0.5) has u = 128 and disparity 128.  e1 is put at 7 (between 5.991 and 7.8): a stereo edge passes, a mono edge fails.
P0, C0 = (-0.125, 0.0, 0.5), (-0.075, 0.0, 0.25)
TRI_MAP0 = [PL(0.5, x=-0.125)]
_mk0 = lambda dv, ur: tri_data(TRI_MAP0, P0, C0, [0], [], ur1=True, ur2=False, dv1=dv, uvr1=None if ur is None else [128.0, 192.0 + dv, ur])
_DV0 = solve(lambda dv: tri_errs(_mk0(dv, None))[0], 7.0, 0.5, 8.0)
for _n, _ur, _ok in (("plus_0", 0.0, 1), ("minus_0", -0.0, 1), ("minus_1", -1.0, 0)):
    TRI("tri_u_right_" + _n, "tri.chi2", "stereo: 7.8 applies" if _ok else "mono: 5.991 applies", _mk0(_DV0, _ur), 0 if _ok else -1)
pair("tri_u_right_minus_0", "tri_u_right_minus_1", "out")
for _s, _t in sides(STR_THR):
    _mk = lambda d, prm=None: tri_data([PL(2.0 + d)], P2, C21, [0], [], ur1=False, ur2=False, prm=prm)
    _d = solve(lambda d: tri_errs(_mk(d))[2], _t, 0.01, 1.0)
    TRI("tri_chi2_str_" + _s, "tri.chi2_str", "within" if _s == "below" else "above", _mk(_d), 0 if _s == "below" else -1, band=dict(thr=STR_THR, side=_s, q=_tri_q(_mk(_d), 2)))
    if _s == "above":
        TRI("tri_chi2_str_above_check_off", "tri.chi2_str", "the check off: accepted", _mk(_d, dict(tri_check_str_chi2=0)), 0)
pair("tri_chi2_str_below", "tri_chi2_str_above", "out")
for _o in (-1, 8):
    TRI("tri_skip_oct1_%s" % str(_o).replace("-", "minus_"), "tri.skip", "not solved", tri_data(TRI_MAP, P2, C21, [0], [], oct1=_o), -1)
TRI("tri_solved_oct1_7", "tri.skip", "solved", tri_data(TRI_MAP, P2, C21, [0], [], oct1=7), 0)

# ================================================ createMapPoints ========================================================================
def cmp_data(uvr1, depth1, uvr2, depth2, c2, comps=None, cand1=(), cand2=(), oct1=0, oct2=0, scale_factor=1.2, cam=CAM5, pose2=None):
    mean, cov = mk_map(comps or [PL(50.0, x=20.0)])
    k = max(len(cand1), len(cand2), 1)
    a, b = -np.ones((1, k), np.int32), -np.ones((1, k), np.int32)
    a[0, :len(cand1)], b[0, :len(cand2)] = cand1, cand2
    p2 = np.concatenate([[0, 0, 0, 1], -np.array(c2, f64)]) if pose2 is None else np.array(pose2, f64)
    return dict(mean=mean, cov=cov, cam=cam, prm={}, scale_factor=scale_factor, pose1=ID7[None].copy(), uvr1=np.array(uvr1, f64)[None], depth1=np.array([depth1], f32),
                oct1=np.array([oct1], np.int32), pose2=p2[None], uvr2=np.array(uvr2, f64)[None], depth2=np.array([depth2], f32), oct2=np.array([oct2], np.int32),
                cand1=a, n1=np.array([len(cand1)], np.int32), cand2=b, n2=np.array([len(cand2)], np.int32))


def CMP(name, decision, side, data, typ, comp_=-1, xzero=None, **kw):
    want = dict(type=np.array([typ], np.int32), comp=np.array([comp_], np.int32))
    if xzero is not None:
        want["xzero"] = np.array([xzero])
    return add(name, "cmp", decision, side, data, want, **kw)


def _cmp_type(data):
    return int(run(numpy_ref, "cmp", data)["type"][0])


# two monocular key-points, key-frame 2 0.1 to the right: the rays (0, 0, 1) and (du / 512, 0, 1) meet at depth -51.2 / du
_mono = lambda du: cmp_data([256.0, 192.0, -1.0], -1.0, [256.0 + du, 192.0, -1.0], -1.0, (0.1, 0, 0))
_a, _b = flip(lambda du: _cmp_type(_mono(du)), f64(-12.0), f64(-9.0))
CMP("cmp_mono_parallax_below_0.9998", "cmp.parallax", "float(cosRays) < 0.9998: triangulated", _mono(_a), 1, xzero=False)
CMP("cmp_mono_parallax_at_0.9998", "cmp.parallax", "the next float: neither branch, zeros", _mono(_b), 0, xzero=True)
pair("cmp_mono_parallax_below_0.9998", "cmp_mono_parallax_at_0.9998", "type")
# stereo on side 1 (depth 5: cosStereo 0.99969): wide rays triangulate, narrow ones unproject the stereo key-point
_st1 = lambda b, **kw: cmp_data([256.0, 192.0, 256.0 - 12.8], 5.0, [256.0 - 512.0 * b / 5.0, 192.0, -1.0], -1.0, (b, 0, 0), **kw)
CMP("cmp_stereo1_wide", "cmp.parallax", "cosRays < cosStereo: triangulated", _st1(0.2), 1, xzero=False)
CMP("cmp_stereo1_narrow", "cmp.parallax", "cosRays >= cosStereo, stereo 1: unprojected", _st1(0.05), 3, xzero=False)
pair("cmp_stereo1_wide", "cmp_stereo1_narrow", "type")
CMP("cmp_stereo2_narrow", "cmp.parallax", "stereo on side 2 only: unprojected from key-frame 2",
    cmp_data([256.0, 192.0, -1.0], -1.0, [256.0 - 5.12, 192.0, 256.0 - 5.12 - 12.8], 5.0, (0.05, 0, 0)), 3, xzero=False)
# both stereo: only depth1 is read; depth2 = 0.3 would give a far lower cosStereo (and a triangulation) were it read
CMP("cmp_stereo_both_depth2_unread", "cmp.parallax", "stereo on both: side 1's depth alone",
    cmp_data([256.0, 192.0, 256.0 - 12.8], 5.0, [256.0 - 5.12, 192.0, 256.0 - 5.12 - 12.8], 0.3, (0.05, 0, 0)), 3, xzero=False)
# rays at 90 degrees exactly: xn1 = (1, 0, 1), xn2 = (-1, 0, 1) on a 2048-wide image, key-frame 2 at (1, 0, 0)
WIDE = dict(CAM5, cx=1024.0, width=2048)
_perp = lambda u2, **kw: cmp_data([1536.0, 192.0, kw.pop("ur1", -1.0)], kw.pop("d1", -1.0), [u2, 192.0, -1.0], -1.0, (1.0, 0, 0), cam=WIDE, **kw)
CMP("cmp_rays_90_degrees", "cmp.parallax", "cosRays = 0: not > 0, zeros", _perp(512.0), 0, xzero=True)
CMP("cmp_rays_below_90_degrees", "cmp.parallax", "cosRays > 0: triangulated", _perp(513.0), 1, xzero=False)
CMP("cmp_rays_beyond_90_degrees", "cmp.parallax", "cosRays < 0: zeros", _perp(511.0), 0, xzero=True)
CMP("cmp_rays_90_degrees_stereo1", "cmp.parallax", "cosRays = 0 with stereo 1: unprojected", _perp(512.0, ur1=1536.0 - 128.0, d1=0.5), 3, xzero=False)
pair("cmp_rays_90_degrees", "cmp_rays_below_90_degrees", "type")
# u_right >= 0 but no depth: stereo for the parallax test (cosStereo from depth -1), so the unprojection branch runs and puts the point behind
_nod = lambda ur: cmp_data([256.0, 192.0, ur], -1.0, [256.0 - 5.12, 192.0, -1.0], -1.0, (0.05, 0, 0))
CMP("cmp_u_right_without_depth", "cmp.depth_vs_uright", "u_right >= 0, depth -1: the stereo branch, a point behind", _nod(243.2), 0, xzero=False)
CMP("cmp_no_u_right_no_depth", "cmp.depth_vs_uright", "monocular: neither branch", _nod(-1.0), 0, xzero=True)
# ... and a monocular edge in the optimisation.  Both key-frames see the point from the depth 2, both key-points carry the u_right of that depth,
# key-point 2 with its depth; key-point 1 is off in v so that both errors are 6.9 (the two share the offset evenly), between 5.991 and 7.8 - at
# the plane and at the triangulated point alike, so the reprojection tests (7.8: u_right >= 0) pass.  Without depth 1 its edge is monocular and
# the plane is rejected; with it the edge is stereo and the plane is taken.
C22 = (0.5, 0.0, 0.0)
_E69 = solve(lambda dv: tri_errs(tri_data(TRI_MAP, P2, C22, [0], [], ur1=False, ur2=True, dv1=dv))[0], 6.9, 0.5, 8.0)


def _edge_kind(depth1):
    t = tri_data(TRI_MAP, P2, C22, [0], [], ur1=True, ur2=True, dv1=_E69)
    return cmp_data(t["uvr1"][0], depth1, t["uvr2"][0], 2.0, C22, comps=TRI_MAP, cand1=[0])


CMP("cmp_u_right_without_depth_mono_edge", "cmp.depth_vs_uright", "u_right >= 0, depth -1: a monocular edge (5.991), the plane rejected", _edge_kind(-1.0), 1, comp_=-1, xzero=False)
CMP("cmp_u_right_with_depth_stereo_edge", "cmp.depth_vs_uright", "u_right >= 0, depth 2: a stereo edge (7.8), the plane taken", _edge_kind(2.0), 2, comp_=0, xzero=False)
# exact image edges: the stereo key-point (u1, 192) at depth 4 unprojects to x = (u1 - 256) / 128 exactly; key-frame 2 is 1/8 to the side
_edge = lambda u1, c, u2: cmp_data([u1, 192.0, u1 - 16.0], 4.0, [u2, 192.0, -1.0], -1.0, (c, 0, 0))
CMP("cmp_project_u2_0", "cmp.project", "u = 0 in key-frame 2: inside", _edge(16.0, 0.125, 0.0), 3, xzero=False)
CMP("cmp_project_u2_width", "cmp.project", "u = width in key-frame 2: outside", _edge(496.0, -0.125, 512.0), 0, xzero=False)
# (a stereo key-point cannot sit at u = 0, its u_right would be negative: for key-frame 1 the point is unprojected from key-frame 2)
_edge2 = lambda u1, c, u2: cmp_data([u1, 192.0, -1.0], -1.0, [u2, 192.0, u2 - 16.0], 4.0, (c, 0, 0))
CMP("cmp_project_u1_0", "cmp.project", "u = 0 in key-frame 1: inside", _edge2(0.0, -0.125, 16.0), 3, xzero=False)
CMP("cmp_project_u1_width", "cmp.project", "u = width in key-frame 1: outside", _edge2(512.0, 0.125, 496.0), 0, xzero=False)
pair("cmp_project_u2_0", "cmp_project_u2_width", "type")
# u_right = 320 is right for the depth -1 the stereo branch unprojects: behind key-frame 1, in front of key-frame 2 at the distance 1, no error anywhere
CMP("cmp_project_behind_1", "cmp.project", "behind key-frame 1", cmp_data([256.0, 192.0, 320.0], -1.0, [256.0, 192.0, -1.0], -1.0, (0, 0, -2.0)), 0, xzero=False)
CMP("cmp_project_behind_2", "cmp.project", "behind key-frame 2", cmp_data([256.0, 192.0, 240.0], 4.0, [256.0, 192.0, -1.0], -1.0, (0, 0, 8.0)), 0, xzero=False)  # (as far behind 2 as before 1: the scale test would pass)
# reprojection: the point unprojected from key-point 1 = (16, 192) at depth 4 reprojects there exactly, with u_right = 0: the error of key-frame 1 is
# u_right^2, set as a float (the reference reads u_right as one; near 2.8 its spacing moves the error by 2e-7 of itself).  Key-point 2 is moved in v.
S2 = [f32(1.0)]
for _ in range(7):
    S2.append(f32(S2[-1] * f32(1.2)))
S2 = [float(f32(s * s)) for s in S2]


def _rep(dv1, dv2, oct1, oct2):
    return cmp_data([16.0, 192.0, float(f32(dv1))], 4.0, [256.0 - 512.0 * 1.925 / 4.0, 192.0 + dv2, -1.0], -1.0, (0.05, 0, 0), oct1=oct1, oct2=oct2)


def _rep_kf2_stereo(dv2, oct1, oct2):
    """both stereo, the point unprojected from key-point 1; key-point 2 = (22.4, 192) with its u_right 6.4, moved in v"""
    return cmp_data([16.0, 192.0, 0.0], 4.0, [22.4, 192.0 + dv2, 6.4], 4.0, (-0.05, 0, 0), oct1=oct1, oct2=oct2)


def _rep_kf1_mono(dv1, oct1, oct2):
    """key-point 1 monocular, the point unprojected from the stereo key-point 2 = (16, 192, 0) at depth 4; key-point 1 = (22.4, 192) moved in v"""
    return cmp_data([22.4, 192.0 + dv1, -1.0], -1.0, [16.0, 192.0, 0.0], 4.0, (0.05, 0, 0), oct1=oct1, oct2=oct2)


def _q_rep(data, which):
    def q(backend):
        x = run(backend, "cmp", data)["x"][0]
        kp, c2 = data["uvr%d" % which][0], -data["pose%d" % which][0][4:]
        pc = x - c2
        u, v = 512.0 * (pc[0] / pc[2]) + 256.0, 512.0 * (pc[1] / pc[2]) + 192.0
        e = (kp[0] - u) ** 2 + (kp[1] - v) ** 2
        return float(e + ((kp[2] - (u - 64.0 / pc[2])) ** 2 if kp[2] >= 0 else 0.0))
    return q


for _o1, _o2 in ((0, 1), (3, 2)):
    for _w, _thr in ((1, 7.8), (2, 5.991)):
        for _s, _t in sides(_thr * S2[_o1]):
            _dv = float(np.sqrt(_t))
            _dat = _rep(_dv, 0.0, _o1, _o2) if _w == 1 else _rep(0.0, _dv, _o1, _o2)
            CMP("cmp_reproj_kf%d_oct%d_%s" % (_w, _o1, _s), "cmp.reproj", "within" if _s == "below" else "above: rejected", _dat, 3 if _s == "below" else 0, xzero=False,
                band=dict(thr=_thr * S2[_o1], side=_s, q=_q_rep(_dat, _w)))
        pair("cmp_reproj_kf%d_oct%d_below" % (_w, _o1), "cmp_reproj_kf%d_oct%d_above" % (_w, _o1), "type")
    for _w, _thr, _mk, _n in ((1, 5.991, _rep_kf1_mono, "kf1_mono"), (2, 7.8, _rep_kf2_stereo, "kf2_stereo")):
        for _s, _t in sides(_thr * S2[_o1]):
            _dat = _mk(float(np.sqrt(_t)), _o1, _o2)
            CMP("cmp_reproj_%s_oct%d_%s" % (_n, _o1, _s), "cmp.reproj", "within" if _s == "below" else "above: rejected", _dat, 3 if _s == "below" else 0, xzero=False,
                band=dict(thr=_thr * S2[_o1], side=_s, q=_q_rep(_dat, _w)))
        pair("cmp_reproj_%s_oct%d_below" % (_n, _o1), "cmp_reproj_%s_oct%d_above" % (_n, _o1), "type")
# scale: the point (0, 0, 1) is 1 from key-frame 1 and d2 from key-frame 2, which sits on the axis
_sc = lambda d2, sf, o1=0, o2=0: cmp_data([256.0, 192.0, 192.0], 1.0, [256.0, 192.0, -1.0], -1.0, (0, 0, 1.0 - float(d2)), scale_factor=sf, oct1=o1, oct2=o2)
CMP("cmp_scale_upper_at_1.25", "cmp.scale", "ratio_dist = ratio_octave * factor: kept", _sc(1.875, 1.25), 3)
CMP("cmp_scale_upper_above_1.25", "cmp.scale", "the next float: rejected", _sc(above(f32(1.875)), 1.25), 0)
pair("cmp_scale_upper_at_1.25", "cmp_scale_upper_above_1.25", "type")
CMP("cmp_scale_upper_octaves_at_1.25", "cmp.scale", "octaves 2 and 0: ratio_octave 1.5625, kept at 2.9296875", _sc(2.9296875, 1.25, 2, 0), 3)
CMP("cmp_scale_upper_octaves_above_1.25", "cmp.scale", "the next float: rejected", _sc(above(f32(2.9296875)), 1.25, 2, 0), 0)
_a, _b = flip(lambda d: _cmp_type(_sc(d, 1.25)), f32(0.5), f32(0.6))
CMP("cmp_scale_lower_below_1.25", "cmp.scale", "ratio_dist * factor < ratio_octave: rejected", _sc(_a, 1.25), 0)
CMP("cmp_scale_lower_at_1.25", "cmp.scale", "the next float: kept", _sc(_b, 1.25), 3)
pair("cmp_scale_lower_below_1.25", "cmp_scale_lower_at_1.25", "type")
_a, _b = flip(lambda d: _cmp_type(_sc(d, 1.2)), f32(1.5), f32(2.0))
CMP("cmp_scale_upper_at_1.2", "cmp.scale", "scale factor 1.2: kept", _sc(_a, 1.2), 3)
CMP("cmp_scale_upper_above_1.2", "cmp.scale", "scale factor 1.2, the next float: rejected", _sc(_b, 1.2), 0)
_a, _b = flip(lambda d: _cmp_type(_sc(d, 1.2)), f32(0.5), f32(0.6))
CMP("cmp_scale_lower_below_1.2", "cmp.scale", "scale factor 1.2: rejected", _sc(_a, 1.2), 0)
CMP("cmp_scale_lower_at_1.2", "cmp.scale", "scale factor 1.2, the next float: kept", _sc(_b, 1.2), 3)
# types
_P5 = [PL(5.0)]
CMP("cmp_type_1", "cmp.type", "1 triangulated", _st1(0.2), 1)
CMP("cmp_type_2", "cmp.type", "2 triangulated, with a component", _st1(0.2, comps=_P5, cand1=[0]), 2, comp_=0)
CMP("cmp_type_3", "cmp.type", "3 stereo", _st1(0.05), 3)
CMP("cmp_type_4", "cmp.type", "4 stereo, with a component", _st1(0.05, comps=_P5, cand2=[0]), 4, comp_=0)
CMP("cmp_type_0", "cmp.type", "0 rejected", _mono(-5.0), 0, xzero=True)

# ================================================ the chain: search2d feeds the point kernels ============================================
# name -> dict(view data of each key-frame, the point call and its data without the candidate tables, the declared outputs)
CHAINS = {}
# the two planes merge in the view (the nearer, index 1, stays); the feature on the axis gets [1]; its refinement stays with 1 (0 is farther)
_cv = CASES[V("chain_view_of_two_planes", "view.merge", "two planes of a stack: the nearer one", [PL(2.012), PL(2.009)], [1], uv=_UV0, k=5, cand=[[1, -1, -1, -1, -1]], ncand=[1])]
CHAINS["search2d_to_check_map_association"] = dict(views=[_cv.data], call="cma", data=cma_data([PL(2.012), PL(2.009)], [1], k=5), cand=[np.array([[1, -1, -1, -1, -1]], np.int32)],
                                                   want=dict(out=np.array([1], np.int32), moved=np.array([True])))
# one plane at depth 5 seen by both key-frames of cmp_type_4: both tables hold it, the stereo point takes it
_d4 = _st1(0.05, comps=_P5, cand1=[0], cand2=[0])
_v1 = dict(mean=_d4["mean"], cov=_d4["cov"], cam=CAM5, pose=_d4["pose1"][0], uv=_d4["uvr1"][:, :2].copy(), k=1, view_cap=None, nfeat=None)
_v2 = dict(_v1, pose=_d4["pose2"][0], uv=_d4["uvr2"][:, :2].copy())
CHAINS["search2d_to_create_map_points"] = dict(views=[_v1, _v2], call="cmp", data=_d4, cand=[np.array([[0]], np.int32), np.array([[0]], np.int32)],
                                               want=dict(type=np.array([4], np.int32), comp=np.array([0], np.int32)))

# ================================================ regime scenes ==========================================================================
def bh2_far(a, b):
    """the screen of k_search2d (gl_view.hip bh2_far) on two (mean2d, cov2d): True = not listed for the exact distance"""
    c = (a[1] + b[1]) / 2.0
    d = b[0] - a[0]
    det, P = c[0, 0] * c[1, 1] - c[1, 0] * c[0, 1], np.linalg.det(a[1]) * np.linalg.det(b[1])
    qa = (d[0] * c[1, 1] - d[1] * c[1, 0]) * d[0] + (d[1] * c[0, 0] - d[0] * c[0, 1]) * d[1]
    return bool(qa > 16.0 * det and det >= 1e-10 * c[0, 0] * c[1, 1] and det > 0 and det * det >= 0.0184 * P)


def near_pairs_of_last_round(m2, c2):
    """An ESTIMATE of the pairs (accepted slot, candidate) a late round of a view lists: MG accepted components against the others, taken
    from the depth-sorted view, which is not the order of the rounds.  It is no bound in general; in the fan every component is near every
    other, so which MG are taken does not matter.  bh2_far restates the device's screen with its constants: if the kernel's screen
    changes, this property has to follow it by hand (the GPU test of the scene compares the output either way)."""
    V_ = len(m2)
    return sum(not bh2_far((m2[i], c2[i]), (m2[j], c2[j])) for j in range(V_ - MG, V_) for i in range(V_ - MG))


def _needle_fan(n=160):
    mean = np.tile(np.array([[0.0, 0.0, 3.0]]), (n, 1)) + np.random.default_rng(5).normal(0, 1e-4, (n, 3))
    cov = np.empty((n, 3, 3))
    for i in range(n):
        a = np.pi * i / n
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        cov[i] = R @ np.diag([0.5 ** 2, 0.002 ** 2, 0.0005 ** 2]) @ R.T
    return mean, cov


def _regime(name, mean, cov, prop, why, pose=ID7, cam=None, n_uv=24):
    rng = np.random.default_rng(len(REGIMES) + 11)
    cam = cam or dict(fx=435.2, fy=435.2, cx=367.45, cy=252.2, bf=47.9, width=752, height=480)
    uv = np.stack([rng.uniform(250, 500, n_uv), rng.uniform(150, 330, n_uv)], 1)
    REGIMES[name] = dict(data=dict(mean=mean, cov=cov, cam=cam, pose=np.array(pose, f64), uv=uv, k=5, view_cap=None, nfeat=None), prop=prop, why=why)


_regime("needle_fan", *_needle_fan(), lambda ids, m2, c2: near_pairs_of_last_round(m2, c2) > 2 * 1024,
        "more near pairs in a round than NEAR_CAP = 2 * T_VIEW of either block shape (512, 2048): the exhaustive path")
# more accepted components than the small view_slot_lds (24) of the device test: the list spills to the global scratch
_regime("long_list", *mk_map([_filler(i) for i in range(40)]), lambda ids, m2, c2: len(ids) == 40, "40 accepted components against view_slot_lds = 24", cam=CAM5)
for _K in (257, 1025):  # K just over one block's stride: the visible components sit at both ends of the index range, the rest is behind the camera
    _c = [plane(0.3 * (i % 7), 0.2 * (i % 5), -1.0 - 0.01 * i) for i in range(_K)]
    for _j, _i in enumerate(list(range(0, 12)) + list(range(_K - 12, _K))):
        _c[_i] = _filler(_j)
    _regime("big_map_%d" % _K, *mk_map(_c), lambda ids, m2, c2, _K=_K: len(ids) == 24 and ids.max() == _K - 1 and ids.min() == 0,
            "K = %d: the compaction of phase 1 crosses a block stride" % _K, cam=CAM5)
