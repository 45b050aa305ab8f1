#!/usr/bin/env python3
"""Times of the local-BA window built on the device and of the local BA that runs from the resident map, one JSON line per run:
    python tools/ba_window_time.py build [reps]   (a) device time of gl_ba_window_build for ONE key-frame (HIP events around back-to-back
                                                  calls) on the EuRoC-sized scene and on the geometric scene of tests/ba_window_scenes.py,
                                                  and of gl_update_connections / gl_ba_window_apply; each checked against
                                                  tests/ba_window_ref.py first
    python tools/ba_window_time.py map [reps]     (b) host to host: api.joint_optimization_from_map on the geometric scene - build, the
                                                  16 bytes of sizes, the BA, the write-back, the erase list's length read back
    python tools/ba_window_time.py host [reps]    (c) the route without the resident map, on the SAME window already flattened (the
                                                  pointer walk left out: a lower bound of the host path): the window's arrays from
                                                  page-locked memory to the device, gl_joint_optimization, poses / points / flags / iters back.
                                                  Uses entry points the parent commit has, so GMMLOC_HIP_LIB may name a build of it.
    python tools/ba_window_time.py all [reps] [out.txt]   every leg in a process of its own with a time limit, (b) and (c) alternated
                                                  three times, stopping at the first failure; the lines are also written to out.txt
Host to host: wall clock around one call that ends in a synchronise, median / min / max.  The map rows the BA changes are restored
before every timed call (outside the timed part), so every repetition optimises the same window."""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
STEP_LIMIT_S = 240


def run_all():
    out = sys.argv[3] if len(sys.argv) > 3 else None
    lines = []
    for leg in ["build"] + ["map", "host"] * 3:
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
from gmmloc_amd import api  # noqa: E402
from tests import ba_window_ref as R  # noqa: E402
from tests import ba_window_scenes as S  # noqa: E402

cam, prm = api.Camera(), api.Params()
ctx = gmmloc_amd.Context(0)


def dev(d):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in d.items() if v is not None}


def events_us(fn, n):
    """device time per call: n calls enqueued back to back between two events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(ctx.stream):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0.record(ctx.stream)
        for _ in range(n):
            fn()
        e1.record(ctx.stream)
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def stats(ts):
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


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


def geometric():
    g = np.load(os.path.join(ROOT, "tests", "golden", "map_v1.npz"))
    gt = np.load(os.path.join(ROOT, "tests", "golden", "gt_sync.npz"))
    m, ba, kf = S.geometric_scene(g["mean"], g["cov"], gt["V1_01_easy"], cam)
    return g["mean"], g["cov"], m, ba, kf


def build_leg():
    res = {"mode": "build", "device": torch.cuda.get_device_name(0), "reps": REPS}
    m, ba, rows = S.scene("euroc")
    scenes = [("euroc", m, ba, int(rows[0]))]
    _, _, m, ba, kf = geometric()
    scenes.append(("geometric", m, ba, kf))
    for name, m, ba, kf in scenes:
        w = R.window_vec(m, ba, kf)
        caps = S.caps_of([w], slack=64)
        md, bd = dev(m), dev(ba)
        row = torch.tensor([kf], dtype=torch.int32, device="cuda")
        slab = api.ba_window_slab(1, *caps)
        api.ba_window_build(ctx, md, bd, row, slab)
        torch.cuda.synchronize()
        ref, _ = R.ba_window_build(m, ba, [kf], {k: np.zeros(tuple(v.shape), api.BA_WINDOW_DTYPES[k]) for k, v in slab.items() if k in api.BA_WINDOW_DTYPES})
        same = all(slab[k].cpu().numpy().tobytes() == ref[k].tobytes() for k in ref)
        assert same, name
        n = max(REPS // 10, 3)
        # the library calls themselves on structs made once: the wrappers' per-tensor validation costs more host time than these
        # kernels run, and back-to-back calls would time the host
        v, dv = api._map_view(md, False)
        bv = api._map_ba_view(bd, v, dv)
        win, _ = api._ba_window(slab, dv)
        conn = api.update_connections(ctx, md, row, Ccap=256)
        p, ref_ = api._ptr, ctypes.byref
        tb = [events_us(lambda: ctx.lib.gl_ba_window_build(ctx.h, ref_(v), ref_(bv), 1, p(row), ref_(win)), 20) for _ in range(n)]
        tc = [events_us(lambda: ctx.lib.gl_update_connections(ctx.h, ref_(v), 1, p(row), 256, p(conn["conn_kf"]), p(conn["conn_w"]), p(conn["n_conn"]),
                                                              None, p(conn["status"])), 20) for _ in range(n)]
        slab["iters"].fill_(1)
        ta = [events_us(lambda: ctx.lib.gl_ba_window_apply(ctx.h, ref_(v), p(md["mp_pos"]), ref_(bv), 1, ref_(win), p(slab["dropped"]), p(slab["erase"]),
                                                           p(slab["iters"]), p(slab["erase_obs"]), p(slab["n_erase"])), 20) for _ in range(n)]
        torch.cuda.synchronize()
        assert all(slab[k].cpu().numpy().tobytes() == ref[k].tobytes() for k in ref), name
        NMP, NKF, NFK, NOBS = R._sizes(m)
        res[name] = {"NMP": NMP, "NKF": NKF, "NFK": NFK, "NOBS": NOBS, "P": w["P"], "F": w["F"], "L": w["L"], "nobs": w["nobs"],
                     "build_device_us_median_min_max": stats(tb), "connections_device_us_median_min_max": stats(tc),
                     "apply_device_us_median_min_max": stats(ta), "equal_to_restatement": bool(same)}
    print(json.dumps(res))


def ba_legs():
    mean, cov, m, ba, kf = geometric()
    g = api.GMM(ctx, mean, cov)
    w = R.window_vec(m, ba, kf)
    P, F, L, nobs = w["P"], w["F"], w["L"], w["nobs"]
    res = {"mode": MODE, "lib": os.path.basename(os.path.dirname(os.path.abspath(os.environ.get("GMMLOC_HIP_LIB", "gmmloc_amd/x")))), "reps": REPS,
           "P": P, "F": F, "L": L, "nobs": nobs}
    if MODE == "map":
        md, bd = dev(m), dev(ba)
        keep = {k: bd[k].clone() for k in ("kf_pose", "kf_twc", "mp_assoc")}
        pos0 = md["mp_pos"].clone()
        slab = api.ba_window_slab(1, P + 4, F + 4, L + 64, nobs + 256)
        out = {}

        def restore():
            for k, v in keep.items():
                bd[k].copy_(v)
            md["mp_pos"].copy_(pos0)

        def call():
            out["r"] = api.joint_optimization_from_map(ctx, g, cam, prm, md, bd, kf, (P + 4, F + 4, L + 64, nobs + 256), slab=slab)
        res["host_to_host_us_median_min_max"] = wall_us(call, restore, REPS)
        r = out["r"]
        res.update(iters=int(r["iters"][0]), n_erase=int(len(r["erase_obs"])), bytes_down=16 + 4 + 4, bytes_up=4)
    elif MODE == "host":
        keys = ("poses", "prior", "points", "assoc", "obs_ptr", "obs_pose", "obs_uvr", "obs_oct")
        pinned = {k: torch.from_numpy(np.ascontiguousarray(w[k][None])).pin_memory() for k in keys}
        d = {k: v.cuda() for k, v in pinned.items()}
        down = {}
        out = {}

        def call():
            for k in keys:  # the flattened window up
                d[k].copy_(pinned[k], non_blocking=True)
            dropped, erase, iters = api.joint_optimization(ctx, g, cam, prm, P, F, d["poses"], d["prior"], d["points"], d["assoc"], d["obs_ptr"],
                                                           d["obs_pose"], d["obs_uvr"], d["obs_oct"])
            for k, t in (("poses", d["poses"]), ("points", d["points"]), ("dropped", dropped), ("erase", erase), ("iters", iters)):  # the results down
                if k not in down:
                    down[k] = torch.empty(t.shape, dtype=t.dtype).pin_memory()
                down[k].copy_(t, non_blocking=True)
            out["iters"] = iters
        res["host_to_host_us_median_min_max"] = wall_us(call, lambda: None, REPS)
        res.update(iters=int(out["iters"][0]), n_erase=int(down["erase"].sum()),
                   bytes_up=int(sum(v.numel() * v.element_size() for v in pinned.values())),
                   bytes_down=int(sum(v.numel() * v.element_size() for v in down.values())))
    else:
        raise SystemExit("mode: build | map | host | all")
    print(json.dumps(res))


if __name__ == "__main__":
    if MODE == "build":
        build_leg()
    else:
        ba_legs()
