#!/usr/bin/env python3
"""Times of createMapPoints on the resident map (gl_create_map_points_from_map), one JSON line per run:
    python tools/create_points_time.py kernels [reps]    (a) device time (HIP events around ONE call) and the launch count of
                                                   gl_create_map_points_from_map for one generated key-frame of 1 200 features with 10
                                                   neighbours (tests/create_points_cases.Generated: 11 key-frames that see the same 1 200
                                                   world points, a map of the points a third of them already hold, a GMM of 24 planes)
    python tools/create_points_time.py composite [reps]  (b) host to host, map_grow.create_map_points_from_map on that key-frame:
                                                   update_connections -> the loop -> map_add (device counts) -> update_map_points on the new
                                                   rows; one read-back of 24 bytes, nothing uploaded
    python tools/create_points_time.py split [reps]      (c) the route it replaces: update_connections and its list read back, F / epipole in
                                                   numpy, per neighbour the two key-frames' tables uploaded, the public search, its matches
                                                   read back, the gather, the per-match block, its types and points read back, the mask
                                                   updated on the host; then the lists uploaded to map_add and update_map_points on the new
                                                   rows.  Uses entry points the parent commit has.  Checked against (b)'s map once, untimed
    python tools/create_points_time.py all [reps] [out.txt]   every leg in a process of its own with a time limit, (b) and (c) alternated
                                                   three times, stopping at the first failure; the lines are also written to out.txt
Host to host: wall clock around one pass that ends in a synchronise, median / min / max; the map is restored before every timed pass
(outside the timed part).  The split route's lists are built by the test model's Python loop (tests/create_points_ref.py), which a C++ host
would do faster: its share is reported separately as host_loop_us."""
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
NFK, NKF, SEED, NN = 1200, 11, 77, 10


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

import torch  # noqa: E402

import gmmloc_amd  # noqa: E402
from gmmloc_amd import api, map_grow  # noqa: E402
from tests import create_points_cases as cc  # noqa: E402
from tests.test_gpu_create_points import BA_KEYS, MAP_KEYS, T as _T, add_lists, resident, split_route  # noqa: E402
from tests.test_gpu_map_grow import refresh  # noqa: E402

ctx = gmmloc_amd.Context(0)


def T(a):
    return _T(torch, a)


def stats(ts):
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


class Scene:
    def __init__(self):
        self.sc = sc = cc.generated(NFK, NKF, SEED)
        self.cam, self.prm = api.Camera(**sc.cam), api.Params()
        self.g = api.GMM(ctx, sc.mean, sc.cov.reshape(-1, 9))
        self.kt = {k: T(v) for k, v in sc.kt.items()}
        self.md, self.bd, self.rk, self.sizes = resident(torch, sc, 2 * NFK, 4 * NFK)
        refresh(ctx, self.md, self.bd, self.rk, self.kt["desc"], self.sizes)
        torch.cuda.synchronize()
        self.keep = [(t, t.clone()) for t in list(self.md.values()) + [v for v in self.bd.values() if hasattr(v, "clone")] + [self.rk]]
        self.mb = map_grow.default_mb(self.cam)
        self.row = T(np.array([0], np.int32))
        self.host_loop_us = []

    def restore(self):
        for t, c in self.keep:
            t.copy_(c)

    def resident(self):
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t, _ in self.keep]

    def view(self):
        m1, b1 = map_grow.map_views(self.md, self.bd, self.sizes)
        return {k: m1[k] for k in MAP_KEYS}, {k: b1[k] for k in BA_KEYS}

    def composite(self):
        return map_grow.create_map_points_from_map(ctx, self.g, self.cam, self.prm, self.md, self.bd, self.kt, 0, nn=NN, sizes=self.sizes, mp_ref_kf=self.rk)

    def split(self):
        NMP = self.sizes[0]
        mv, _ = self.view()
        cn = api.update_connections(ctx, mv, self.row, Ccap=NN)
        conn, n_conn = cn["conn_kf"][0].cpu().numpy(), int(cn["n_conn"][0])  # (the first read-back)
        t = time.perf_counter()
        s = split_route(torch, ctx, self.sc, conn, n_conn, 0, NN, self.mb, NMP, None)
        self.host_loop_us.append(1e6 * (time.perf_counter() - t))
        r = add_lists(torch, ctx, self.md, self.bd, self.rk, self.sizes, s)
        n = s["n_new"]
        if n and not r["status"]:
            m2, b2 = r["map"], r["ba"]
            new = slice(NMP, NMP + n)
            api.update_map_points(ctx, dict(twc=b2["kf_twc"], valid=m2["kf_valid"], oct=b2["kf_oct"], desc=self.kt["desc"]),
                                  dict(pos=m2["mp_pos"][new], valid=m2["mp_valid"][new], ref_kf=self.rk[new], obs_ptr=m2["obs_ptr"][NMP:], obs_kf=m2["obs_kf"],
                                       obs_feat=b2["obs_feat"]),
                                  dict(desc=m2["mp_desc"][new], normal=m2["mp_normal"][new], max_dist=m2["mp_max_dist"][new], min_dist=m2["mp_min_dist"][new]))
        r["n_new"] = n
        r["nb_stats"] = s["nb_stats"]
        return r


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
    s = Scene()
    mv, bv = s.view()
    cn = api.update_connections(ctx, mv, s.row, Ccap=NN)
    out = map_grow.tri_points_out(NFK, NN)
    call = lambda: map_grow.create_map_points_on_map(ctx, s.g, s.cam, s.prm, mv, bv, s.kt, 0, cn["conn_kf"][0], cn["n_conn"], n_nb=NN, mb=s.mb, mp_base=s.sizes[0], out=out)
    ts = []
    with torch.cuda.stream(ctx.stream):
        for i in range(REPS + 3):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            call()
            e1.record(ctx.stream)
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(1e3 * e0.elapsed_time(e1))
    print(json.dumps({"mode": "kernels", "device": torch.cuda.get_device_name(0), "reps": REPS, "NFK": NFK, "nn": NN, "k": 5, "n_new": int(out["n_new"][0]),
                      "nb_stats": out["nb_stats"][:, :5].tolist(), "launches": 2 + 6 * NN, "device_us_median_min_max": stats(ts)}))


def pass_legs():
    s = Scene()
    NMP, nkf, NOBS = s.sizes
    res = {"mode": MODE, "reps": REPS, "NMP": NMP, "NKF": nkf, "NFK": NFK, "NOBS": NOBS, "nn": NN}
    a = s.composite()
    after_a = s.resident()
    s.restore()
    b = s.split()
    assert a["status"] == 0 and b["status"] == 0 and a["n_new"] == b["n_new"] and after_a == s.resident(), "the two routes differ"
    s.restore()
    s.host_loop_us = []
    res.update(n_new=int(a["n_new"]), attached=a["n_attached"], nb_stats=np.asarray(b["nb_stats"])[:, :5].tolist())
    res["host_to_host_us_median_min_max"] = wall_us(s.composite if MODE == "composite" else s.split, s.restore, REPS)
    if MODE == "split":
        res["per_neighbour_loop_us_median_min_max"] = stats(s.host_loop_us[5:])
    print(json.dumps(res))


if __name__ == "__main__":
    if MODE == "kernels":
        kernels_leg()
    elif MODE in ("composite", "split"):
        pass_legs()
    else:
        raise SystemExit("mode: kernels | composite | split | all")
