#!/usr/bin/env python3
"""Times of the resident covisibility graph and of searchInNeighbors on it, one JSON line per run:
    python tools/covis_time.py kernels [reps]    (a) device time (HIP events around ONE call each, the graph restored before it) of the
                                                 five calls on the EuRoC-sized map of tests/map_edit_scenes.py (1.41 M observations), the
                                                 graph built by gl_covis_update over its key-frames in row order: gl_covis_update of the
                                                 key-frame with the longest list, gl_covis_remove of three rows, gl_covis_best (N = 10),
                                                 gl_fuse_targets (10 + up to 50) and gl_fuse_candidates on its targets
    python tools/covis_time.py composite [reps]  (b) host to host: covis.search_in_neighbors_from_map on the geometric scene of
                                                 tests/map_grow_scenes.py (the EuRoC-sized map carries no descriptors to fuse on)
    python tools/covis_time.py split [reps]      (c) the route it replaces on the same scene: the graph and the two lists kept in numpy
                                                 from read-backs (tests/covis_ref.py), the same fuse calls per target
    python tools/covis_time.py all [reps] [out.txt]   every leg in a process of its own with a time limit, (b) and (c) alternated three
                                                 times, stopping at the first failure; the lines are also written to out.txt
Host to host: wall clock around one pass that ends in a synchronise, median / min / max; the scene is uploaded afresh before every timed
pass (outside the timed part)."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
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
from gmmloc_amd import api, covis  # noqa: E402
from tests import covis_ref as R  # noqa: E402

ctx = gmmloc_amd.Context(0)
GRAPH = ("cov_kf", "cov_w", "cov_n", "cov_nord", "best_cov")


def stats(ts):
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def event_us(fn, restore, n):
    """device time of ONE call between two events, n times"""
    ts = []
    with torch.cuda.stream(ctx.stream):
        for i in range(n + 3):
            restore()
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


def kernels_leg():
    from tests import map_edit_scenes as ES
    from tests.covis_dev import dev_map
    sc = ES.scene("euroc", "euroc" in ES.CLAMP)
    m = sc["m"]
    NKF, NFK = m["kf_mp"].shape
    md = dev_map(torch, m)
    g = covis.covis_alloc(NKF, 64)
    for k in range(NKF):  # (outside any timing: one read per call, the tables re-strided when a row outgrows them)
        _, g = covis.update_connections_in_map(ctx, md, g, k, Ccap=8)
    torch.cuda.synchronize()
    keep = {k: g[k].clone() for k in GRAPH}
    host = {k: g[k].cpu().numpy() for k in GRAPH}
    kf = int(np.argmax(host["cov_nord"]))
    rm = host["cov_kf"][kf, :3].astype(np.int32)

    def restore():
        for k in GRAPH:
            g[k].copy_(keep[k])
    v, dev = api._map_view(md, False)
    s = covis._cov(g, dev)[0]
    p, ref_ = api._ptr, C.byref
    Z = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
    Ccap, Tcap = 64, 60
    conn_kf, conn_w, n_conn, result = Z(Ccap), Z(Ccap), Z(1), Z(4)
    rows, row1 = torch.from_numpy(rm).cuda(), torch.tensor([kf], dtype=torch.int32, device="cuda")
    tgt, n_tgt = Z(Tcap), Z(1)
    cand, n_cand = Z(Tcap * NFK), Z(1)
    res = {"mode": "kernels", "device": torch.cuda.get_device_name(0), "reps": REPS, "NMP": len(m["mp_valid"]), "NKF": int(NKF), "NFK": int(NFK),
           "NOBS": len(m["obs_kf"]), "Wcap": int(g["cov_kf"].shape[1]), "kf_row": kf, "cov_n": int(host["cov_n"][kf]), "cov_nord": int(host["cov_nord"][kf])}
    res["update_device_us_median_min_max"] = event_us(
        lambda: ctx.lib.gl_covis_update(ctx.h, ref_(v), ref_(s), kf, Ccap, p(conn_kf), p(conn_w), p(n_conn), p(result)), restore, REPS)
    res["update_result"] = result.tolist()
    res["remove_device_us_median_min_max"] = event_us(lambda: ctx.lib.gl_covis_remove(ctx.h, int(NKF), ref_(s), -1, p(rows), None, len(rm), p(result)), restore, REPS)
    res["remove_rows"], res["remove_result"] = rm.tolist(), result.tolist()
    restore()
    res["best_device_us_median_min_max"] = event_us(
        lambda: ctx.lib.gl_covis_best(ctx.h, int(NKF), ref_(s), 1, p(row1), 10, Ccap, p(conn_kf), p(conn_w), p(n_conn), p(result)), lambda: None, REPS)
    res["targets_device_us_median_min_max"] = event_us(
        lambda: ctx.lib.gl_fuse_targets(ctx.h, int(NKF), ref_(s), p(md["kf_valid"]), kf, 10, 5, Tcap, p(tgt), p(n_tgt), p(result)), lambda: None, REPS)
    res["n_tgt"] = int(n_tgt.item())
    res["candidates_device_us_median_min_max"] = event_us(
        lambda: ctx.lib.gl_fuse_candidates(ctx.h, ref_(v), p(tgt), p(n_tgt), Tcap, 5, Tcap * int(NFK), p(cand), p(n_cand), p(result)), lambda: None, REPS)
    res["n_cand"] = int(n_cand.item())
    # checked against the numpy statement of the row representation
    want_t = R.rows_targets(host, NKF, m["kf_valid"], kf, 10, 5, Tcap)
    want_c = R.rows_candidates(m, want_t["tgt_kf"], int(want_t["n_tgt"][0]), 5, Tcap * NFK)
    res["equal_to_model"] = bool(np.array_equal(tgt.cpu().numpy(), want_t["tgt_kf"]) and np.array_equal(cand.cpu().numpy(), want_c["cand_mp"]))
    assert res["equal_to_model"]
    print(json.dumps(res))


def pass_legs():
    from tests import map_grow_scenes as GS
    from tests.test_gpu_covis import _scene, _split_route
    gold = os.path.join(ROOT, "tests", "golden")
    d = np.load(os.path.join(gold, "map_v1.npz"))
    sc = GS.geo_scene(d["mean"], d["cov"], np.load(os.path.join(gold, "gt_sync.npz"))["V1_01_easy"])
    cam = api.Camera()
    K = sc["kf_row"]
    ts, info = [], {}
    for i in range(REPS + 3):
        s = _scene(torch, ctx, sc)
        NMP, NKF, NOBS = s["sizes"]  # (on entry)
        torch.cuda.synchronize()
        t = time.perf_counter()
        if MODE == "composite":
            r = covis.search_in_neighbors_from_map(ctx, cam, s["md"], s["bd"], s["cov"], dict(desc=s["kf_desc"]), K, 5, stats=s["stats"], mp_replaced=s["rep"],
                                                   mp_ref_kf=s["rk"], sizes=s["sizes"])
            torch.cuda.synchronize()
            info = dict(n_tgt=len(r["tgt_kf"]), n_cand=r["n_cand"], fused=int(sum(r["n_fused"])), replaced=int(sum(r["n_replaced"])))
        elif MODE == "split":
            targets, cand, counts, _ = _split_route(torch, ctx, cam, s, K, 5)
            torch.cuda.synchronize()
            info = dict(n_tgt=len(targets), n_cand=len(cand), fused=int(sum(c[0] for c in counts)), replaced=int(sum(c[2] for c in counts)))
        else:
            raise SystemExit("mode: kernels | composite | split | all")
        if i >= 3:
            ts.append(1e6 * (time.perf_counter() - t))
    print(json.dumps(dict(mode=MODE, reps=REPS, scene="geo_scene", NMP=NMP, NKF=NKF, NOBS=NOBS, host_to_host_us_median_min_max=stats(ts), **info)))


if __name__ == "__main__":
    if MODE == "kernels":
        kernels_leg()
    else:
        pass_legs()
