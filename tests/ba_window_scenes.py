"""The scenes of tests/test_ba_window_ref.py (CPU: the conditions that keep the GPU tests from passing vacuously) and
tests/test_gpu_ba_window.py (GPU: gl_update_connections / gl_ba_window_build / gl_ba_window_apply against tests/ba_window_ref.py), with
pinned seeds.  Test infrastructure; nothing in the product imports it."""
import os

import numpy as np

from gmmloc_amd import api, synth
from tests import ba_window_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- structural scenes on synth.synth_chain_map: name -> (map seed, NMP, NKF, NFK, B).  tiny / small / euroc: the maps of
# tests/local_map_scenes.py::UPDATE_SCENES (every window of `tiny` takes the single-largest branch; `small` has weight ties and invalid
# key-frames in its lists; `euroc` is the size of a EuRoC session's map); the others sit on either side of the bound of the
# per-key-frame words in LDS (4 096 key-frames) and of 2^20 map points (the bound of gl_update_local_map's mask: nothing changes
# here at it, which is what the scenes show).  "clique": a few key-frames that all share at least 15 points, so F = 0.
SCENES = {
    "tiny": (11, 300, 40, 24, 16),
    "small": (12, 6000, 150, 300, 16),
    "euroc": (13, 180000, 1500, 1200, 2),
    "kf_at_bound": (14, 30000, 4096, 40, 16),
    "kf_over_bound": (15, 30000, 4097, 40, 16),
    "mp_at_bound": (16, 1 << 20, 2000, 600, 2),
    "mp_over_bound": (17, (1 << 20) + 1, 2000, 600, 2),
    "clique": (18, 0, 6, 64, 6),
}
SMALL = ("tiny", "small", "clique")


def _obs_feat(m):
    """the feature index of every CSR entry: the slot of the observing key-frame that holds the point"""
    NMP, NKF, NFK, NOBS = R._sizes(m)
    k, s = np.nonzero(m["kf_mp"] >= 0)
    key = k.astype(np.int64) * max(NMP, 1) + m["kf_mp"][k, s]
    by = np.argsort(key, kind="stable")
    pt = np.repeat(np.arange(NMP), np.diff(m["obs_ptr"]))
    want = m["obs_kf"].astype(np.int64) * max(NMP, 1) + pt
    at = np.searchsorted(key[by], want)
    assert len(key) and (key[by][np.minimum(at, len(key) - 1)] == want).all(), "the CSR and kf_mp disagree"
    return s[by][at].astype(np.int32)


def _isolate(m, e):
    """key-frame e loses its part in the map: its slots hold points nobody else observes (an EMPTY counter), the CSR forgets it elsewhere"""
    pt = np.repeat(np.arange(len(m["obs_ptr"]) - 1), np.diff(m["obs_ptr"]))
    own = np.zeros(len(m["obs_ptr"]) - 1, bool)
    held = m["kf_mp"][e][m["kf_mp"][e] >= 0][:3]  # three points stay, observed by e alone
    own[held] = True
    keep = np.where(own[pt], m["obs_kf"] == e, m["obs_kf"] != e)
    gone = np.isin(m["kf_mp"], held)
    gone[e] = ~gone[e]
    m["kf_mp"][gone] = -1
    m["obs_kf"] = m["obs_kf"][keep]
    ptr = np.zeros(len(m["obs_ptr"]), np.int64)
    ptr[1:] = np.cumsum(np.bincount(pt[keep], minlength=len(own)))
    m["obs_ptr"] = ptr.astype(np.int32)


def _clique(rng, NKF, NFK):
    """NKF key-frames that all hold the same 30 points (each in a slot of its own choice), + 10 private points each"""
    NMP = 30 + 10 * NKF
    kf_mp = -np.ones((NKF, NFK), np.int32)
    obs = [[] for _ in range(NMP)]
    for k in range(NKF):
        slots = rng.permutation(NFK)[:40]
        pts = np.concatenate([np.arange(30), 30 + 10 * k + np.arange(10)])
        kf_mp[k, slots] = pts
        for p in pts:
            obs[p].append(k)
    obs = [list(rng.permutation(o)) for o in obs]
    ptr = np.zeros(NMP + 1, np.int32)
    ptr[1:] = np.cumsum([len(o) for o in obs])
    m = dict(mp_valid=np.ones(NMP, np.uint8), obs_ptr=ptr, obs_kf=np.array([k for o in obs for k in o], np.int32), kf_valid=np.ones(NKF, np.uint8),
             kf_mp=kf_mp, mp_pos=rng.uniform(-5, 5, (NMP, 3)))
    m["mp_valid"][[3, 31]] = 0
    m["kf_valid"][NKF - 1] = 0
    return m


def scene(name):
    """-> (map dict (the keys of gl_map_view that the calls read), ba dict, kf_rows (B,) int32)"""
    seed, NMP, NKF, NFK, B = SCENES[name]
    rng = np.random.default_rng(seed + 4242)
    if name == "clique":
        m = _clique(rng, NKF, NFK)
        NMP = len(m["mp_valid"])
        rows = np.arange(B, dtype=np.int32) % NKF
    else:
        full = synth.synth_chain_map([], seed, NMP, NKF, NFK)["map"]
        m = {k: full[k] for k in ("mp_valid", "obs_ptr", "obs_kf", "kf_valid", "kf_mp", "mp_pos")}
        rows = rng.choice(NKF, B, replace=False).astype(np.int32)
        if B >= 16:
            _isolate(m, int(rows[1]))
            m["kf_valid"][rows[1]] = 1
            m["mp_valid"][m["kf_mp"][rows[1]][m["kf_mp"][rows[1]] >= 0]] = 1
            rows[5] = rows[4]  # the same key-frame twice in a batch
    NOBS = len(m["obs_kf"])
    q = rng.standard_normal((NKF, 4))
    ba = dict(kf_pose=np.concatenate([q / np.linalg.norm(q, axis=1)[:, None], rng.uniform(-5, 5, (NKF, 3))], 1),
              kf_twc=rng.uniform(-5, 5, (NKF, 3)), kf_uvr=rng.uniform(0, 480, (NKF, NFK, 3)), kf_oct=rng.integers(0, 8, (NKF, NFK)).astype(np.int32),
              obs_feat=_obs_feat(m), mp_assoc=np.where(rng.uniform(size=NMP) < 0.6, rng.integers(0, 3000, NMP), -1).astype(np.int32),
              kf_first=int(rows[0]) if name != "tiny" else int(m["obs_kf"][0]))
    mono = rng.uniform(size=(NKF, NFK)) < 0.2
    ba["kf_uvr"][mono, 2] = -1.0
    assert len(ba["obs_feat"]) == NOBS
    return m, ba, rows


def malform(m, ba, seed):
    """rows outside the tables in kf_mp, obs_kf and obs_feat, CSR ranges outside [0, NOBS] - in place (on copies the caller made)"""
    NMP, NKF, NFK, NOBS = R._sizes(m)
    rng = np.random.default_rng(seed)
    at = rng.uniform(size=m["kf_mp"].shape) < 0.02
    m["kf_mp"][at] = rng.choice(np.array([NMP, NMP + 5, 2 ** 31 - 1, -2, -2 ** 31], np.int64), int(at.sum()))
    at = rng.uniform(size=NOBS) < 0.02
    m["obs_kf"][at] = rng.choice(np.array([NKF, NKF + 3, 2 ** 31 - 1, -1, -2 ** 31], np.int64), int(at.sum()))
    at = rng.uniform(size=NOBS) < 0.02
    ba["obs_feat"][at] = rng.choice(np.array([NFK, NFK + 1, 2 ** 31 - 1, -1, -2 ** 31], np.int64), int(at.sum()))
    pts = rng.choice(NMP, 60, replace=False)
    m["obs_ptr"][pts] = rng.choice(np.array([-1, NOBS + 1, 2 ** 31 - 1, -2 ** 31], np.int64), 60)


def caps_of(wins, slack=8):
    """capacities from the restatement's windows: the largest of each size + slack"""
    ws = [w for w in wins if w is not None]
    return tuple(max([w[k] for w in ws] + [1]) + slack for k in ("P", "F", "L", "nobs"))


def empty_slab(B, caps, fill=-7):
    """the numpy arrays of api.ba_window_slab, every entry a sentinel"""
    Pcap, Fcap, Lcap, Ocap = caps
    shapes = {"poses": (B, Pcap + Fcap, 7), "prior": (B, Pcap), "points": (B, Lcap, 3), "assoc": (B, Lcap), "obs_ptr": (B, Lcap + 1),
              "obs_pose": (B, Ocap), "obs_uvr": (B, Ocap, 3), "obs_oct": (B, Ocap), "win_kf": (B, Pcap + Fcap), "win_mp": (B, Lcap),
              "win_obs": (B, Ocap), "sizes": (B, 4), "status": (B,)}
    return {k: np.full(sh, 77 if k == "prior" else fill, api.BA_WINDOW_DTYPES[k]) for k, sh in shapes.items()}


def window_kinds(m, ba, rows, wins=None):
    """per window, from the restatement alone -> dict of bool arrays (B,)"""
    _, kfv = R._valid(m)
    kinds = {k: np.zeros(len(rows), bool) for k in ("tie", "single", "empty", "invalid_conn", "invalid_observer", "shared_point", "mono", "f0", "f_pos")}
    for b, kf in enumerate(rows):
        c = R.connections_seq(m, int(kf))
        w = R.window_seq(m, ba, int(kf)) if wins is None else wins[b]
        kinds["empty"][b] = c["empty"]
        kinds["single"][b] = not c["empty"] and c["conn_w"][0] < R.TH
        kinds["tie"][b] = len(c["conn_w"]) >= 2 and (np.diff(c["conn_w"]) == 0).any()
        kinds["invalid_conn"][b] = (~kfv[c["conn_kf"]]).any()
        kinds["mono"][b] = (w["obs_uvr"][:, 2] < 0).any()
        kinds["f0"][b], kinds["f_pos"][b] = w["F"] == 0 and w["L"] > 0, w["F"] > 0
        free = w["win_kf"][:w["P"]]
        held = m["kf_mp"][free].ravel()
        held = held[held >= 0]
        kinds["shared_point"][b] = len(np.unique(held)) < len(held)
        for p in w["win_mp"]:
            ks = m["obs_kf"][m["obs_ptr"][p]:m["obs_ptr"][p + 1]]
            if (~kfv[ks]).any():
                kinds["invalid_observer"][b] = True
                break
    return kinds


# ---- the geometric scene: a stretch of the V1_01_easy trajectory, points drawn from the map's components, observations by projection
GEO = dict(seed=31, first=900, step=6, NKF=24, NFK=140, per_kf=70, kf_row=4, assoc_frac=0.7, mono_frac=0.2)


def geometric_scene(mean, cov, gt, cam=None):
    """-> (map dict, ba dict, kf_row).  Key-frames on every GEO['step']-th gt_sync row; per key-frame GEO['per_kf'] points drawn from the
    components it sees; every point is observed by the key-frames that see it (depth 0.3 - 8 m, inside the image), as long as they have
    a free slot; pixel noise by octave, a share of monocular observations; mp_assoc = the point's own component for a share of them;
    poses and points start a little off (as tests/test_gpu_ba.py::make_ba_problem); one key-frame and a few points invalid."""
    cam = api.Camera() if cam is None else cam
    g = GEO
    rng = np.random.default_rng(g["seed"])
    NKF, NFK, K = g["NKF"], g["NFK"], mean.shape[0]
    Ts = [synth.gt_row_to_Tcw(gt[g["first"] + i * g["step"]]) for i in range(NKF)]

    def project(T, X):
        pc = X @ synth.quat_to_R(T[:4]).T + T[4:]
        z = np.where(np.abs(pc[:, 2]) < 1e-9, 1e-9, pc[:, 2])
        u, v = cam.fx * pc[:, 0] / z + cam.cx, cam.fy * pc[:, 1] / z + cam.cy
        return u, v, z, (z > 0.3) & (z < 8.0) & (u >= 0) & (u < cam.width) & (v >= 0) & (v < cam.height)
    comp = []
    for T in Ts:
        vis = np.nonzero(project(T, mean)[3])[0]
        comp.append(vis[rng.integers(0, len(vis), g["per_kf"])])
    comp = np.concatenate(comp)
    NMP = len(comp)
    Lc = np.linalg.cholesky(cov.reshape(K, 3, 3)[comp] + 1e-15 * np.eye(3))
    X = mean[comp] + np.einsum("nij,nj->ni", Lc, rng.standard_normal((NMP, 3)))
    kf_mp = -np.ones((NKF, NFK), np.int32)
    kf_uvr = np.zeros((NKF, NFK, 3))
    kf_oct = np.zeros((NKF, NFK), np.int32)
    obs = [[] for _ in range(NMP)]
    for k, T in enumerate(Ts):
        u, v, z, ok = project(T, X)
        seen = rng.permutation(np.nonzero(ok)[0])[:NFK]
        slots = rng.permutation(NFK)[:len(seen)]
        octv = rng.integers(0, 5, len(seen))
        sig = 1.2 ** octv * 0.8
        uu, vv = u[seen] + rng.standard_normal(len(seen)) * sig, v[seen] + rng.standard_normal(len(seen)) * sig
        ur = uu - cam.bf / z[seen] + rng.standard_normal(len(seen)) * sig * 0.5
        ur[rng.uniform(size=len(seen)) < g["mono_frac"]] = -1.0
        kf_mp[k, slots] = seen
        kf_uvr[k, slots] = np.stack([uu, vv, ur.astype(np.float32).astype(np.float64)], 1)
        kf_oct[k, slots] = octv
        for p, s in zip(seen, slots):
            obs[p].append((k, s))
    obs = [[o[i] for i in rng.permutation(len(o))] for o in obs]  # in no particular order
    ptr = np.zeros(NMP + 1, np.int32)
    ptr[1:] = np.cumsum([len(o) for o in obs])
    m = dict(mp_valid=(rng.uniform(size=NMP) >= 0.02).astype(np.uint8), obs_ptr=ptr, obs_kf=np.array([k for o in obs for k, _ in o], np.int32),
             kf_valid=np.ones(NKF, np.uint8), kf_mp=kf_mp, mp_pos=X + rng.standard_normal((NMP, 3)) * 0.01)
    m["kf_valid"][g["kf_row"] + 2] = 0
    pose = np.stack([synth.perturb_pose(T, rng, 0.004, 0.015) for T in Ts])
    ba = dict(kf_pose=pose, kf_twc=np.stack([R.twc_of(p) for p in pose]), kf_uvr=kf_uvr, kf_oct=kf_oct,
              obs_feat=np.array([s for o in obs for _, s in o], np.int32),
              mp_assoc=np.where(rng.uniform(size=NMP) < g["assoc_frac"], comp, -1).astype(np.int32), kf_first=0)
    return m, ba, g["kf_row"]
