#!/usr/bin/env python3
"""Times of the resident map's found / visible counters and of removeMapPoints on the device, one JSON line per run:
    python tools/map_stats_time.py calls [reps]   device time of each of the five calls (HIP events around calls enqueued back to back):
                                                  gl_map_stats_track on one tracked frame's outputs and on a batch of 256,
                                                  gl_map_stats_new_points and gl_map_cand_append of 1 200 rows, gl_map_stats_merge of
                                                  200 and of 2 500 steps, gl_cull_map_points of 4 096 candidates, on the EuRoC-sized
                                                  map of tests/map_edit_scenes.py (180 000 points, 1 500 key-frames)
    python tools/map_stats_time.py a|b [reps]     ONE tracked frame (1 200 features, the frame and the map of tools/local_map_time.py A),
                                                  host to host - the wall clock around work that ends in a synchronise:
       a  gl_track_frame_chain_map + gl_map_stats_track, one synchronise
       b  the route without the counters on the device: gl_track_frame_chain_map, then inview, feat_mp, match_local, outlier and
          local_mp copied back (page-locked, one synchronise) and the counters incremented in numpy on the host's mirror
    python tools/map_stats_time.py run [reps]     `calls`, then a and b alternated three times, EACH RUN A PROCESS OF ITS OWN under its
                                                  own time limit, stopping at the first failure; prints every line and the verdict on
                                                  the two legs' intervals (the min .. max of the three medians).
No number is promised: where the intervals of a and b overlap the verdict says so."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODE = sys.argv[1] if len(sys.argv) > 1 else "run"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
NF, NL, NP0 = 1200, 1000, 3000
NMP, NKF, NFK, KFCAP = 12000, 1500, 1200, 128


def orchestrate():
    lines = []

    def child(mode, limit):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, str(REPS)], cwd=ROOT, capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            print("FAILED %s (exit %d), nothing more is started:\n%s" % (mode, r.returncode, r.stderr[-2000:]))
            raise SystemExit(1)
        d = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(d))
        sys.stdout.flush()
        return d
    child("calls", 420)
    med = {"a": [], "b": []}
    for _ in range(3):
        for leg in ("a", "b"):
            med[leg].append(child(leg, 240)["host_to_host_us_median_min_max"][0])
    ia, ib = (min(med["a"]), max(med["a"])), (min(med["b"]), max(med["b"]))
    print("tracked frame, host to host, us, the three medians per leg: a (counters on the device) %s  b (copied back, numpy) %s" %
          (" ".join("%.1f" % v for v in med["a"]), " ".join("%.1f" % v for v in med["b"])))
    if ia[1] < ib[0]:
        print("the intervals do not overlap: a %.1f .. %.1f us < b %.1f .. %.1f us (%.1f%% at the nearest ends)" % (ia + ib + (100 * (ia[1] / ib[0] - 1),)))
    else:
        print("the intervals overlap or a is slower (a %.1f .. %.1f us, b %.1f .. %.1f us): no latency win is claimed" % (ia + ib))


if MODE == "run":
    orchestrate()
    raise SystemExit(0)

import torch  # noqa: E402

import gmmloc_amd  # noqa: E402
from gmmloc_amd import api, map_stats, synth  # noqa: E402

cam, prm = api.Camera(), api.Params()
ctx = gmmloc_amd.Context(0)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def events_us(fn, n, reset=None):
    """device time per call: n calls enqueued back to back between two events (reset: enqueued before each call, timed on its own and
    subtracted)"""
    def window(body):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(ctx.stream):
            for _ in range(5):
                body()
            torch.cuda.synchronize()
            e0.record(ctx.stream)
            for _ in range(n):
                body()
            e1.record(ctx.stream)
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n
    if reset is None:
        return window(fn)
    both = window(lambda: (reset(), fn()))
    return both - window(reset)


def med3(fn, n=20, reset=None):
    ts = [events_us(fn, n, reset) for _ in range(max(REPS // 10, 3))]
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def tracked_frame():
    """the frame and the map of tools/local_map_time.py A -> (the chain's inputs, the map, the lists)"""
    from tests.test_gpu_chain import pack
    f = synth.synth_chain_frame(NF, NL, NP0, 7000, cam)
    s = synth.synth_chain_map([f], 31, NMP, NKF, NFK)
    NPcap = 4096
    blank = dict(f)
    blank.update(mp_pos=np.zeros((NPcap, 3)), mp_normal=np.zeros((NPcap, 3)), mp_max_dist=np.zeros(NPcap, np.float32), mp_min_dist=np.zeros(NPcap, np.float32),
                 mp_cand=np.zeros(NPcap, np.uint8), mp_desc=np.zeros((NPcap, 32), np.uint8), last_to_local=-np.ones(NL, np.int32))
    a = {k: v for k, v in pack(torch, [blank]).items() if k not in api.CHAIN_MAP_IGNORED}
    md = {k: T(v) for k, v in s["map"].items() if v is not None}
    lm = api.local_map_lists(1, KFCAP, NPcap)
    lm["last_mp"] = T(s["last_mp"][0][None])
    return a, md, lm


def calls():
    from tests import map_edit_scenes as ES
    from tests import map_stats_cases as SC
    res = {"mode": "calls", "device": torch.cuda.get_device_name(0), "reps": REPS}
    a, md, lm = tracked_frame()
    st = map_stats.map_stats_alloc(NMP, 8192)
    out = api.track_frame_chain_map(ctx, cam, prm, a, md, lm)
    torch.cuda.synchronize()
    args = (out["feat_mp"], out["match_local"], out["outlier"], out["inview"], lm["local_mp"], lm["n_local_mp"], out["counts2"])
    res["track_b1_device_us_median_min_max"] = med3(lambda: map_stats.map_stats_track(ctx, st, NMP, *args))
    res["track_b1_rows_held_inview"] = [int((out["feat_mp"] >= 0).sum()), int(out["inview"].sum())]
    big = [t.expand(256, *t.shape[1:]).contiguous() for t in args]
    res["track_b256_device_us_median_min_max"] = med3(lambda: map_stats.map_stats_track(ctx, st, NMP, *big))
    ref_kf = T(np.random.default_rng(1).integers(0, NKF, 1200).astype(np.int32))
    res["new_points_1200_device_us_median_min_max"] = med3(lambda: map_stats.map_stats_new_points(ctx, st, NKF, NMP - 1200, ref_kf))
    zero = lambda: st["n_cand"].zero_()
    res["cand_append_1200_device_us_median_min_max"] = med3(lambda: map_stats.map_cand_append(ctx, st, rows=ref_kf), reset=zero)
    rng = np.random.default_rng(2)
    for n in (200, 2500):
        src, tgt = T(rng.integers(0, NMP, n).astype(np.int32)), T(rng.integers(0, NMP, n).astype(np.int32))
        res["merge_%d_device_us_median_min_max" % n] = med3(lambda: map_stats.map_stats_merge(ctx, st, NMP, src, tgt))
    sc = ES.scene("euroc")
    c = SC.random_case(sc, np.random.default_rng(3), 4096)
    n_big = len(sc["m"]["mp_valid"])
    cand = np.random.default_rng(4).integers(0, n_big, 4096).astype(np.int32)
    mdd = {k: T(sc["m"][k]) for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")}
    bdd = {k: T(sc["ba"][k]) for k in ("kf_uvr", "obs_feat")}
    st2 = dict(visible=T(c["visible"]), found=T(c["found"]), ref_idx=T(c["ref_idx"]), kf_idx=None if c["kf_idx"] is None else T(c["kf_idx"]),
               cand=T(cand), n_cand=T(np.array([4096], np.int32)))
    cand0 = st2["cand"].clone()
    outs = map_stats.cull_map_points(ctx, mdd, bdd, st2, c["kf_row"])
    torch.cuda.synchronize()
    res["cull_4096_kept_removed_erased"] = outs["result"].cpu().tolist()[:3]
    reset = lambda: (st2["cand"].copy_(cand0), st2["n_cand"].fill_(4096))
    res["cull_4096_of_%d_points_device_us_median_min_max" % n_big] = med3(lambda: map_stats.cull_map_points(ctx, mdd, bdd, st2, c["kf_row"], out=outs), reset=reset)
    print(json.dumps(res))


def wall_us(fn, n):
    ts = []
    with torch.cuda.stream(ctx.stream):
        for i in range(n + 10):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            if i >= 10:
                ts.append(1e6 * (time.perf_counter() - t))
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def leg(which):
    a, md, lm = tracked_frame()
    res = {"mode": which, "reps": REPS}
    if which == "a":
        st = map_stats.map_stats_alloc(NMP, 16)

        def call():
            map_stats.track_frame_with_stats(ctx, cam, prm, a, md, lm, st)
            torch.cuda.synchronize()
    else:
        NPcap = lm["local_mp"].shape[1]
        pinned = dict(inview=torch.empty((1, NPcap), dtype=torch.uint8).pin_memory(), feat_mp=torch.empty((1, NF), dtype=torch.int32).pin_memory(),
                      match_local=torch.empty((1, NF), dtype=torch.int32).pin_memory(), outlier=torch.empty((1, NF), dtype=torch.uint8).pin_memory(),
                      local_mp=torch.empty((1, NPcap), dtype=torch.int32).pin_memory(), n_local_mp=torch.empty((1,), dtype=torch.int32).pin_memory())
        vis, fnd = np.zeros(NMP, np.int32), np.zeros(NMP, np.int32)

        def call():
            out = api.track_frame_chain_map(ctx, cam, prm, a, md, lm)
            for k, h in pinned.items():
                h.copy_(out[k] if k in out else lm[k], non_blocking=True)
            torch.cuda.synchronize()
            fm, ml, lmp = pinned["feat_mp"].numpy()[0], pinned["match_local"].numpy()[0], pinned["local_mp"].numpy()[0]
            np.add.at(vis, fm[fm >= 0], 1)
            n = min(int(pinned["n_local_mp"][0]), NPcap)
            np.add.at(vis, lmp[:n][pinned["inview"].numpy()[0, :n] != 0], 1)
            r = np.where(ml >= 0, lmp[np.clip(ml, 0, NPcap - 1)], fm)
            np.add.at(fnd, r[(pinned["outlier"].numpy()[0] == 0) & (r >= 0)], 1)
    res["host_to_host_us_median_min_max"] = wall_us(call, REPS)
    print(json.dumps(res))


if MODE == "calls":
    calls()
elif MODE in ("a", "b"):
    leg(MODE)
else:
    raise SystemExit("mode: run | calls | a | b")
