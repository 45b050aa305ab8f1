#!/usr/bin/env python3
"""Times of the device updateLocalMap and of the tracked frame that contains it, one JSON line per run:
    python tools/local_map_time.py update [reps]     device time of gl_update_local_map alone (HIP events around back-to-back calls) on a
                                                     small map, a EuRoC-sized one (B = 1, B = 256) and one beyond both LDS bounds;
                                                     each shape checked against tests/local_map_ref.py first
    python tools/local_map_time.py A|B|C [reps]      ONE tracked frame (1 200 features, 1 000 last-frame points, the shape of
                                                     tools/chain_time.py) embedded in a map of 12 000 points / 1 500 key-frames (a local map of ~3 400 points: stage 3 takes at most 4 096):
       A  gl_track_frame_chain_map: updateLocalMap and the gather on the device, one call
       B  gl_track_frame_chain_front -> the copies the host form needs (matches and dropped matches down; the re-flattened local map and
          last_to_local up, from page-locked memory) -> gl_track_frame_chain_back, with NOTHING computed on the host in between: a
          lower bound of what the two halves cost a real host
       C  gl_track_frame_chain on a fixed list: the price of A's extra steps
     B and C run on the local map A's sequence makes for this frame (same list, same order, unpadded), so stage 3 and 4 do the same
     work in all three; they use entry points the parent commit has, so GMMLOC_HIP_LIB may name a build of it (one library per process).
     Host to host: wall clock around one call that ends in a synchronise, median; device: HIP events around calls enqueued back to
     back (B: the two halves' own event intervals, the copies and the gap between them left out).  A and C also as a batch of 2 048."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gmmloc_amd
from gmmloc_amd import api, synth
from tests import local_map_ref as R

MODE = sys.argv[1] if len(sys.argv) > 1 else "update"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
cam, prm = api.Camera(), api.Params()
ctx = gmmloc_amd.Context(0)
NF, NL, NP0 = 1200, 1000, 3000
NMP, NKF, NFK, KFCAP = 12000, 1500, 1200, 128


def dev(d, keys=None):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items() if v is not None and (keys is None or k in keys)}


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


def wall_us(fn, n):
    """host to host: one call and a synchronise, n times -> (median, min, max)"""
    ts = []
    with torch.cuda.stream(ctx.stream):
        for i in range(n + 5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 5:
                ts.append(1e6 * (time.perf_counter() - t))
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def update_shapes():
    from tests import local_map_scenes as S
    res = {"mode": "update", "device": torch.cuda.get_device_name(0), "reps": REPS}
    for name in ("small", "euroc_b1", "euroc_b256", "both_over_bound"):
        m, feat_mp, lists = S.update_scene(name)
        ref = R.update_local_map(m, feat_mp, lists)
        md, fm0, l0 = dev(m, ("mp_valid", "obs_ptr", "obs_kf", "kf_valid", "kf_mp")), torch.from_numpy(feat_mp).cuda(), dev(lists)
        fm, ld = fm0.clone(), {k: v.clone() for k, v in l0.items()}
        api.update_local_map(ctx, md, fm, ld)
        torch.cuda.synchronize()
        same = np.array_equal(fm.cpu().numpy(), ref[0]) and all(np.array_equal(ld[k].cpu().numpy(), ref[1][k]) for k in ref[1])
        assert same, name
        ts = [events_us(lambda: api.update_local_map(ctx, md, fm, ld), 20) for _ in range(max(REPS // 10, 3))]
        seed, nmp, nkf, nfk, B, nf, _, _ = S.UPDATE_SCENES[name]
        res[name] = {"NMP": nmp, "NKF": nkf, "NFK": nfk, "B": B, "NF": nf, "local_kf_mean": float(ref[1]["n_local_kf"].mean()),
                     "local_mp_mean": float(ref[1]["n_local_mp"].mean()), "device_us_per_call_median_min_max": [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))],
                     "equal_to_restatement": bool(same)}
    print(json.dumps(res))


def frame_scene():
    """the frame, its map, and the local map A's sequence makes for it (through the restatement, from the front half's matches)"""
    from tests.test_gpu_chain import pack
    f = synth.synth_chain_frame(NF, NL, NP0, 7000, cam)
    s = synth.synth_chain_map([f], 31, NMP, NKF, NFK)
    blank = dict(f)
    blank.update(mp_pos=np.zeros((1, 3)), mp_normal=np.zeros((1, 3)), mp_max_dist=np.zeros(1, np.float32), mp_min_dist=np.zeros(1, np.float32),
                 mp_cand=np.zeros(1, np.uint8), mp_desc=np.zeros((1, 32), np.uint8), last_to_local=-np.ones(NL, np.int32))
    front = api.track_frame_chain_front(ctx, cam, prm, pack(torch, [blank]), th_mm=7.0)
    torch.cuda.synchronize()
    ml = front["match_last"].cpu().numpy()[0]
    fm, ml2, _ = R.derive_feat_mp(s["map"], ml, -np.ones_like(ml), s["last_mp"][0], None, 0)
    r = R.frame_vec(s["map"], fm)
    n = len(r["local_mp"])
    g = dict(f)
    g.update(R.gather_local_map(s["map"], r["local_mp"], n, n, s["last_mp"][0]))
    return f, s, g, n, pack


def main():
    if MODE == "update":
        return update_shapes()
    f, s, g, n, pack = frame_scene()
    NPcap = ((n + 255) // 256) * 256
    res = {"mode": MODE, "lib": os.path.basename(os.path.dirname(os.path.abspath(os.environ.get("GMMLOC_HIP_LIB", "gmmloc_amd/x")))), "reps": REPS,
           "n_local_mp": n, "NPcap": NPcap}
    BIG = 2048
    if MODE == "A":
        a = {k: v for k, v in pack(torch, [g]).items() if k not in api.CHAIN_MAP_IGNORED}
        md = dev(s["map"])
        lm = api.local_map_lists(1, KFCAP, NPcap)
        lm["last_mp"] = torch.from_numpy(s["last_mp"][0][None]).cuda()
        call = lambda: api.track_frame_chain_map(ctx, cam, prm, a, md, lm)
        out = call()
        torch.cuda.synchronize()
        assert int(lm["n_local_mp"][0]) == n and int(lm["status"][0]) == 0
        res["stage3_matches"] = int(out["counts"][0, 2])
        big = {k: v.expand(BIG, *v.shape[1:]).contiguous() for k, v in a.items()}
        lmb = api.local_map_lists(BIG, KFCAP, NPcap)
        lmb["last_mp"] = lm["last_mp"].expand(BIG, NL).contiguous()
        callb = lambda: api.track_frame_chain_map(ctx, cam, prm, big, md, lmb)
    elif MODE == "C":
        a = pack(torch, [g])
        out = api.track_frame_chain(ctx, cam, prm, a)
        call = lambda: api.track_frame_chain(ctx, cam, prm, a)
        torch.cuda.synchronize()
        res["stage3_matches"] = int(out["counts"][0, 2])
        big = {k: v.expand(BIG, *v.shape[1:]).contiguous() for k, v in a.items()}
        callb = lambda: api.track_frame_chain(ctx, cam, prm, big)
    elif MODE == "B":
        a = pack(torch, [g])
        up_keys = ("mp_pos", "mp_normal", "mp_max_dist", "mp_min_dist", "mp_cand", "mp_desc", "last_to_local")
        pinned_up = {k: a[k].cpu().pin_memory() for k in up_keys}
        pinned_down = {k: torch.empty((1, NF), dtype=torch.int32).pin_memory() for k in ("match_last", "drop_src")}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        seg = []

        def call():
            ev[0].record(ctx.stream)
            front = api.track_frame_chain_front(ctx, cam, prm, a)
            ev[1].record(ctx.stream)
            for k, h in pinned_down.items():
                h.copy_(front[k], non_blocking=True)
            torch.cuda.synchronize()  # the host reads the matches: updateLocalMap would run here
            for k in up_keys:
                a[k].copy_(pinned_up[k], non_blocking=True)
            ev[2].record(ctx.stream)
            out = api.track_frame_chain_back(ctx, cam, prm, a, front)
            ev[3].record(ctx.stream)
            torch.cuda.synchronize()
            seg.append(1e3 * (ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3])))
            return out
        with torch.cuda.stream(ctx.stream):
            out = call()
        res["stage3_matches"] = int(out["counts"][0, 2])
        res["bytes_down_up"] = [int(sum(h.numel() * h.element_size() for h in pinned_down.values())), int(sum(h.numel() * h.element_size() for h in pinned_up.values()))]
        callb = None
    else:
        raise SystemExit("mode: update | A | B | C")
    res["host_to_host_us_median_min_max"] = wall_us(call, REPS)
    if MODE == "B":
        res["device_us_median_min_max"] = [float(np.median(seg[-REPS:])), float(np.min(seg[-REPS:])), float(np.max(seg[-REPS:]))]
    else:
        ts = [events_us(call, 20) for _ in range(max(REPS // 10, 3))]
        res["device_us_median_min_max"] = [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]
    if callb is not None:
        callb()
        torch.cuda.synchronize()
        tb = [events_us(callb, 3) for _ in range(3)]
        res["batch_2048_ms_median"] = float(np.median(tb)) / 1e3
        res["batch_2048_frames_per_s"] = BIG / (float(np.median(tb)) * 1e-6)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
