#!/usr/bin/env python3
"""Times of the depth-ordered walks (gl_create_stereo_points, gl_create_temporal_points) and of a key-frame's GMM half on the resident
map, one JSON line per run:
    python tools/key_frame_create_time.py kernels [reps]   (a) device time (HIP events around ONE call each) of both entry points on seeded
                                                   random key-frames of NF = 1 200 features on map_v1, k = 5, B = 1 and B = 64; the B = 1
                                                   outputs checked against the sequential model on the device's own check results first
    python tools/key_frame_create_time.py composite [reps] (b) host to host, one key-frame of the geometric scene of
                                                   tests/test_gpu_key_frame_create.py through map_grow.process_key_frame_from_map:
                                                   search2d -> create_stereo_points -> map_add (device counts) -> update_map_points on the
                                                   new rows; one read-back of 24 bytes, nothing uploaded
    python tools/key_frame_create_time.py split [reps]     (c) the route without the call: search2d, the candidate counts read back, the host
                                                   sorts by depth, unprojects and masks (numpy, vectorised), gl_check_map_association, its
                                                   answers and points read back, the host walks (numpy, vectorised - the walk a C++ host
                                                   would do in a loop), the lists uploaded, map_add, update_map_points on the new rows.
                                                   Uses entry points the parent commit has.  Checked against (b)'s map once, untimed
    python tools/key_frame_create_time.py all [reps] [out.txt]   every leg in a process of its own with a time limit, (b) and (c) alternated
                                                   three times, stopping at the first failure; the lines are also written to out.txt
Host to host: wall clock around one pass that ends in a synchronise, median / min / max; the map is restored before every timed pass
(outside the timed part)."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 30
STEP_LIMIT_S = 240


def run_all():
    out = sys.argv[3] if len(sys.argv) > 3 else None
    lines = []
    for leg in ["kernels"] + ["composite", "split"] * 3:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), leg, str(REPS)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("leg %s failed (exit status %d): stopping" % (leg, r.returncode))
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if MODE == "all":
    run_all()
    raise SystemExit(0)

import ctypes as C  # noqa: E402

import torch  # noqa: E402

import gmmloc_amd  # noqa: E402
from gmmloc_amd import _lib, api, map_grow  # noqa: E402
from tests import key_frame_create_ref as ref  # noqa: E402
from tests.test_gpu_key_frame_create import key_frame_scene, random_key_frame, split_route  # noqa: E402
from tests.test_gpu_map_grow import refresh, upload, with_point_arrays  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ctx = gmmloc_amd.Context(0)
f32, f64 = np.float32, np.float64


def T(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a, dt))).cuda()


def stats(ts):
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def map_v1():
    d = np.load(os.path.join(GOLDEN, "map_v1.npz"))
    return d["mean"], d["cov"]


def event_us(fn, n):
    """device time of ONE call between two events, n times"""
    ts = []
    with torch.cuda.stream(ctx.stream):
        for i in range(n + 3):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            rc = fn()
            e1.record(ctx.stream)
            torch.cuda.synchronize()
            assert rc == 0, rc
            if i >= 3:
                ts.append(1e3 * e0.elapsed_time(e1))
    return stats(ts)


def wall_us(fn, restore, n):
    ts = []
    with torch.cuda.stream(ctx.stream):
        for i in range(n + 5):
            restore()
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 5:
                ts.append(1e6 * (time.perf_counter() - t))
    return stats(ts)


def kernels_leg():
    mean, cov = map_v1()
    cam, prm = api.Camera(), api.Params()
    camd = dict(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
    g = api.GMM(ctx, mean, cov)
    gt = np.load(os.path.join(GOLDEN, "gt_sync.npz"))["V1_01_easy"]
    th = float(f32(35.0 * cam.bf / cam.fx))
    NF, k = 1200, 5
    frames = [random_key_frame(torch, ctx, g, cam, mean, cov, gt, NF, 31 + s, k) for s in range(8)]
    res = {"mode": "kernels", "device": torch.cuda.get_device_name(0), "reps": REPS, "NF": NF, "k": k, "th_depth": th}
    p, byref = api._ptr, C.byref
    for B in (1, 64):
        fr = [frames[b % 8] for b in range(B)]
        a = {key: T(np.stack([f[key] for f in fr])) for key in api.STEREO_IN_DTYPES if key != "kf_row"}
        a["kf_row"] = T(np.arange(B, dtype=np.int32))
        out = api.create_stereo_points(ctx, g, cam, prm, a, 9000, 1, th, want_pts0=True)
        torch.cuda.synchronize()
        if B == 1:  # the outputs are the model's on the device's own check results
            o = {key: v[0].cpu().numpy() for key, v in out.items()}
            m = split_route(torch, ctx, g, dict(camd, bf=cam.bf, width=cam.width, height=cam.height), fr, [o["pts0"]], [0], 9000, 1, th)[0][0]
            n = int(o["n_new"])
            assert n == m["n_new"] and np.array_equal(o["stats"], m["stats"]) and np.array_equal(o["feat_new"], m["feat_new"]) and \
                o["new_pos"][:n].tobytes() == m["new_pos"].tobytes() and np.array_equal(o["new_assoc"][:n], m["new_assoc"])
            res["stats_B1"] = o["stats"].tolist()
        si, so = _lib.gl_stereo_points_in(), _lib.gl_stereo_points_out()
        for key in api.STEREO_IN_DTYPES:
            setattr(si, key, p(a[key]))
        for key, v in out.items():
            setattr(so, key, p(v))
        res["stereo_B%d_device_us_median_min_max" % B] = event_us(
            lambda: ctx.lib.gl_create_stereo_points(ctx.h, g.h, byref(cam.c()), byref(prm.c()), B, NF, k, byref(si), 9000, 1, th, byref(so)), REPS)
        rng = np.random.default_rng(5)
        tin = {key: a[key] for key in ("pose", "feat_uv", "feat_depth", "feat_oct", "held")}
        tin.update(last_outlier=T((rng.uniform(size=(B, NF)) < 0.1).astype(np.uint8)), feat_desc=T(rng.integers(0, 256, (B, NF, 32), dtype=np.uint8)))
        last = dict(last_pt=torch.zeros((B, NF, 3), dtype=torch.float64, device="cuda"), last_observed=torch.ones((B, NF), dtype=torch.uint8, device="cuda"),
                    last_valid=torch.ones((B, NF), dtype=torch.uint8, device="cuda"), last_desc=torch.zeros((B, NF, 32), dtype=torch.uint8, device="cuda"))
        t = api.create_temporal_points(ctx, cam, tin, last, th)
        torch.cuda.synchronize()
        if B == 1:
            res["temporal_stats_B1"] = t["stats"][0].tolist()
        ti, to = _lib.gl_temporal_points_in(), _lib.gl_temporal_points_out()
        for key in api.TEMPORAL_IN_DTYPES:
            setattr(ti, key, p(tin[key]))
        for key, v in dict(t, **last).items():
            setattr(to, key, p(v))
        res["temporal_B%d_device_us_median_min_max" % B] = event_us(
            lambda: ctx.lib.gl_create_temporal_points(ctx.h, byref(cam.c()), B, NF, byref(ti), th, byref(to)), REPS)
    print(json.dumps(res))


def host_walk(fr, comp, pts, mp_base, check_depth, th, kf_row):
    """createMapPointsFromStereo's loop on the check's answers, vectorised: what tests/key_frame_create_ref.stereo_walk does entry by entry"""
    depth, held, ncand = fr["feat_depth"], fr["held"], fr["ncand"]
    ent = np.nonzero((depth > 0) & (fr["feat_oct"] >= 0) & (fr["feat_oct"] <= 7))[0]
    ent = ent[np.lexsort((ent, depth[ent]))]
    create = held[ent] != 1
    rejected = create & (ncand[ent] > 0) & (comp[ent] < 0)
    num = np.cumsum(~rejected)
    brk = np.nonzero(~rejected & (depth[ent] > f32(th)) & (num > 100))[0] if check_depth else []
    walked = brk[0] + 1 if len(brk) else len(ent)
    made = ent[:walked][(create & ~rejected)[:walked]]
    n = len(made)
    # (the check wrote only where it ran: elsewhere pts still holds the unprojected point)
    return dict(new_feat=made.astype(np.int32), new_pos=pts[made], new_assoc=comp[made].astype(np.int32), new_ref_kf=np.full(n, kf_row, np.int32),
                att_mp=(mp_base + np.arange(n)).astype(np.int32), n_new=n)


def unproject_all(cam, pose, uv, depth):
    """Frame::unproject3 for every slot, vectorised, in the operation order of tests/key_frame_create_ref.unproject"""
    q, t = ref.twc_of(pose)
    z = depth.astype(f64)
    v = np.stack([z * (uv[:, 0] - cam.cx) / cam.fx, z * (uv[:, 1] - cam.cy) / cam.fy, z], 1)
    x, y, zq, w = q
    u = np.stack([y * v[:, 2] - zq * v[:, 1], zq * v[:, 0] - x * v[:, 2], x * v[:, 1] - y * v[:, 0]], 1)
    u = u + u
    return np.stack([v[:, 0] + w * u[:, 0] + (y * u[:, 2] - zq * u[:, 1]), v[:, 1] + w * u[:, 1] + (zq * u[:, 0] - x * u[:, 2]),
                     v[:, 2] + w * u[:, 2] + (x * u[:, 1] - y * u[:, 0])], 1) + t


class Scene:
    def __init__(self):
        mean, cov = map_v1()
        gt = np.load(os.path.join(GOLDEN, "gt_sync.npz"))
        self.sc, m0, ba0, self.K, self.held, self.depth, self.cam = key_frame_scene((mean, cov), gt)
        self.g = api.GMM(ctx, mean, cov)
        self.th = float(f32(35.0 * self.cam.bf / self.cam.fx))
        NMP, NOBS = len(m0["mp_valid"]), len(m0["obs_kf"])
        self.kf_desc = T(self.sc["kf_desc"])
        self.md, self.bd, self.rk, self.sizes = upload(torch, with_point_arrays(m0, NMP + 400), ba0, self.sc["mp_ref_kf"], NMP + 400, NOBS + 400)
        refresh(ctx, self.md, self.bd, self.rk, self.kf_desc, self.sizes)
        torch.cuda.synchronize()
        self.keep = [(t, t.clone()) for t in list(self.md.values()) + [v for v in self.bd.values() if hasattr(v, "clone")] + [self.rk]]
        self.depth_d, self.held_d = T(self.depth), T(self.held)
        # the key-frame's rows as the host holds them anyway
        self.uvr = self.bd["kf_uvr"][self.K].cpu().numpy()
        self.pose = self.bd["kf_pose"][self.K].cpu().numpy()
        self.oct = self.bd["kf_oct"][self.K].cpu().numpy()
        self.pose_d, self.uv_d = T(self.pose[None]), T(self.uvr[None, :, :2])
        self.uvr_d, self.oct_h = T(self.uvr[None]), self.oct

    def restore(self):
        for t, c in self.keep:
            t.copy_(c)

    def resident(self):
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t, _ in self.keep]

    def composite(self):
        return map_grow.process_key_frame_from_map(ctx, self.g, self.cam, api.Params(), self.md, self.bd, dict(desc=self.kf_desc), self.K, self.depth_d, self.held_d,
                                                   self.th, sizes=self.sizes, mp_ref_kf=self.rk)

    def split(self):
        cam, K, NMP = self.cam, self.K, self.sizes[0]
        cand, ncand, _, _ = self.g.search2d(cam, self.pose_d, self.uv_d, k=5)
        nc = ncand[0].cpu().numpy()  # (the first read-back: the host needs the counts to mask)
        run = (self.depth > 0) & (self.oct_h >= 0) & (self.oct_h <= 7) & (self.held != 1) & (nc > 0)
        pts0 = np.where(((self.depth > 0) & (self.oct_h >= 0) & (self.oct_h <= 7))[:, None], unproject_all(cam, self.pose, self.uvr[:, :2], self.depth), 0.0)
        pts = T(pts0[None])
        comp = api.check_map_association(ctx, self.g, cam, api.Params(), self.pose_d, pts, self.uvr_d, T(np.where(run, self.oct_h, -1).astype(np.int32)[None]), cand, ncand)
        comp_h, pts_h = comp[0].cpu().numpy(), pts[0].cpu().numpy()  # (the second)
        fr = dict(feat_depth=self.depth, feat_oct=self.oct_h, held=self.held, ncand=nc)
        w = host_walk(fr, comp_h, pts_h, NMP, 1, self.th, K)
        r = map_grow.map_add(ctx, self.md, self.bd, self.sizes, new_mp=dict(pos=T(w["new_pos"]), assoc=T(w["new_assoc"]), ref_kf=T(w["new_ref_kf"])),
                             new_kf=T(np.array([K], np.int32)), attach=dict(mp=T(w["att_mp"]), kf=T(w["new_ref_kf"]), feat=T(w["new_feat"])), mp_ref_kf=self.rk)
        n = w["n_new"]
        if n and not r["status"]:
            m2, b2 = r["map"], r["ba"]
            new = slice(NMP, NMP + n)
            api.update_map_points(ctx, dict(twc=b2["kf_twc"], valid=m2["kf_valid"], oct=b2["kf_oct"], desc=self.kf_desc),
                                  dict(pos=m2["mp_pos"][new], valid=m2["mp_valid"][new], ref_kf=self.rk[new], obs_ptr=m2["obs_ptr"][NMP:], obs_kf=m2["obs_kf"],
                                       obs_feat=b2["obs_feat"]),
                                  dict(desc=m2["mp_desc"][new], normal=m2["mp_normal"][new], max_dist=m2["mp_max_dist"][new], min_dist=m2["mp_min_dist"][new]))
        r["n_new"] = n
        return r


def pass_legs():
    s = Scene()
    NMP, NKF, NOBS = s.sizes
    res = {"mode": MODE, "reps": REPS, "NMP": NMP, "NKF": NKF, "NFK": int(s.md["kf_mp"].shape[1]), "NOBS": NOBS}
    # both routes leave the same map (checked once, untimed)
    a = s.composite()
    after_a = s.resident()
    s.restore()
    b = s.split()
    assert a["status"] == 0 and b["status"] == 0 and a["n_new"] == b["n_new"] and after_a == s.resident(), "the two routes differ"
    s.restore()
    res.update(n_new=int(a["n_new"]), stats=a["stats"].tolist(), attached=a["n_attached"])
    res["host_to_host_us_median_min_max"] = wall_us(s.composite if MODE == "composite" else s.split, s.restore, REPS)
    n = int(a["n_new"])
    NFK = res["NFK"]
    res.update(bytes_up=4 if MODE == "composite" else NFK * 28 + n * 48 + 4, bytes_down=24 if MODE == "composite" else 24 + NFK * 32)
    print(json.dumps(res))


if __name__ == "__main__":
    if MODE == "kernels":
        kernels_leg()
    elif MODE in ("composite", "split"):
        pass_legs()
    else:
        raise SystemExit("mode: kernels | composite | split | all")
