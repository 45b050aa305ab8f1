#!/usr/bin/env python3
"""Times of the frame end and the hand-over on the device, one JSON line per run:
    python tools/frame_step_time.py calls [reps]   device time of gl_track_frame_end (with the key-frame rule) and gl_track_frame_next
                                                   (with the descriptor gather) for one frame of 1 200 features on the map of
                                                   tools/local_map_time.py A: HIP events around 20 calls that are enqueued while the
                                                   stream is still busy with earlier work, so that the wrappers' host time is hidden and
                                                   the interval is the kernels' own, launch gaps included (`enqueue_hidden` says that
                                                   the first event had not completed when the last call was enqueued); beside it the
                                                   host's time to enqueue one call
    python tools/frame_step_time.py a|b [reps]     ONE non-key frame to the inputs of the next (1 200 features), host to host - the wall
                                                   clock around work that ends in a synchronise:
       a  frame_step.track_frame_step (chain + counters, frame_end, frame_next, create_temporal_points), one synchronise, stat (8 int32)
          copied back
       b  today's route: the chain + counters, every per-feature output copied back (page-locked, one synchronise), the loop over the
          features in numpy on the host's mirror of the map (tests/frame_step_glue.py), the next frame's rows uploaded,
          create_temporal_points, one synchronise
    python tools/frame_step_time.py run [reps]     `calls`, then a and b alternated three times, EACH RUN A PROCESS OF ITS OWN under its
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
NF, NP0 = 1200, 3000
NMP, NKF, NFK, KFCAP, NPCAP = 12000, 1500, 1200, 128, 4096
TH_DEPTH = 3.5
RULE = dict(num_kfs=3, frame_idx=100, kf_frame_idx=90, fps=20.0, is_idle=1, n_queue=0)


def orchestrate():
    def child(mode, limit):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, str(REPS)], cwd=ROOT, capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            print("FAILED %s (exit %d), nothing more is started:\n%s" % (mode, r.returncode, r.stderr[-2000:]))
            raise SystemExit(1)
        d = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(d))
        sys.stdout.flush()
        return d
    child("calls", 300)
    med = {"a": [], "b": []}
    for _ in range(3):
        for leg_ in ("a", "b"):
            med[leg_].append(child(leg_, 240)["host_to_host_us_median_min_max"][0])
    ia, ib = (min(med["a"]), max(med["a"])), (min(med["b"]), max(med["b"]))
    print("one non-key frame to the next, host to host, us, the three medians per leg: a (the hand-over on the device) %s  b (copied back, numpy, uploaded) %s" %
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
from gmmloc_amd import api, frame_step, key_frame, map_stats, synth  # noqa: E402

cam, prm = api.Camera(), api.Params()
ctx = gmmloc_amd.Context(0)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


BUSY = None  # two 4096 x 4096 fp32 matrices: a few products keep the stream busy for milliseconds


def events_us(fn, n):
    """-> (device us per call, the host's us to enqueue one, whether the enqueueing was hidden behind the work before the first event)"""
    global BUSY
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(ctx.stream):
        if BUSY is None:
            BUSY = (torch.randn(4096, 4096, device="cuda"), torch.empty(4096, 4096, device="cuda"))
        for _ in range(5):
            fn()
        torch.mm(BUSY[0], BUSY[0], out=BUSY[1])
        torch.cuda.synchronize()
        for _ in range(12):
            torch.mm(BUSY[0], BUSY[0], out=BUSY[1])
        e0.record(ctx.stream)
        t = time.perf_counter()
        for _ in range(n):
            fn()
        host = 1e6 * (time.perf_counter() - t) / n
        e1.record(ctx.stream)
        hidden = not e0.query()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n, host, hidden


def med3(fn, n=20):
    """-> ([median, min, max] of the device us per call, the median enqueue us, all windows hidden)"""
    ts = [events_us(fn, n) for _ in range(max(REPS // 10, 3))]
    dev = [t[0] for t in ts]
    return [float(np.median(dev)), float(np.min(dev)), float(np.max(dev))], float(np.median([t[1] for t in ts])), all(t[2] for t in ts)


def scene():
    """one frame of 1 200 features whose last frame has as many, the map of tools/local_map_time.py A with the arrays the hand-over reads
    -> (first state, the frame's buffers, the map, ba, the host's mirror of both)"""
    from tests import frame_step_scenes as S
    f = synth.synth_chain_frame(NF, NF, NP0, 7000, cam)
    s = synth.synth_chain_map([f], 31, NMP, NKF, NFK)
    m, ba = s["map"], S.ba_of(s["map"], 31)
    md = {k: T(v) for k, v in m.items() if v is not None}
    bd = dict({k: T(ba[k]) for k in ("kf_pose", "kf_uvr", "kf_oct", "obs_feat")}, kf_first=0)
    first = {k: T(np.asarray(f[k])[None]) for k in ("pose_lw", "pose_cw", "last_pt", "last_valid", "last_observed", "last_oct", "last_angle", "last_desc")}
    state = frame_step.first_state(first, T(s["last_mp"][0][None]), api.local_map_lists(1, KFCAP, NPCAP))
    frame = {k: T(np.asarray(f[k])[None]) for k in frame_step.FRAME_KEYS if k != "feat_depth"}
    frame["feat_depth"] = T(S._depth(f["feat_uv"], f["feat_ur"], cam)[None])
    return state, frame, md, bd, m, ba


def calls():
    res = {"mode": "calls", "device": torch.cuda.get_device_name(0), "reps": REPS, "features": NF}
    state, frame, md, bd, m, ba = scene()
    st = map_stats.map_stats_alloc(NMP, 16)
    begun = frame_step.track_frame_begin(ctx, cam, prm, state, frame, md, bd, st, TH_DEPTH, rule=frame_step.kf_rule(**RULE))
    new, r = frame_step.track_frame_finish(ctx, cam, state, frame, md, bd, begun, TH_DEPTH)
    torch.cuda.synchronize()
    res["stat"] = begun["end"]["stat"].cpu().tolist()[0]
    res["held_rows_temporal_points"] = [int((r["next"]["held_mp"] >= 0).sum()), int(r["temporal"]["n_temp"][0])]
    rule = frame_step.kf_rule(**RULE)
    chain, lm = begun["chain"], begun["lm"]
    end = med3(lambda: frame_step.frame_end(ctx, md, bd, chain, lm, frame["feat_depth"], TH_DEPTH, last_observed=state["last_observed"], rule=rule,
                                            out=begun["end"]))
    held0 = begun["end"]["held_mp"].clone()
    nxt = med3(lambda: frame_step.frame_next(ctx, md, bd, chain["pose"], state["pose_lw"], lm["ref_kf"], held0, out=r["next"]))
    res["frame_end_device_us_median_min_max"], res["frame_end_enqueue_us"] = end[:2]
    res["frame_next_device_us_median_min_max"], res["frame_next_enqueue_us"] = nxt[:2]
    res["enqueue_hidden"] = bool(end[2] and nxt[2])
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
    state, frame, md, bd, m, ba = scene()
    st = map_stats.map_stats_alloc(NMP, 16)
    rule = frame_step.kf_rule(**RULE)
    res = {"mode": which, "reps": REPS}
    if which == "a":
        stat = torch.empty((1, 8), dtype=torch.int32).pin_memory()

        def call():
            new, r = frame_step.track_frame_step(ctx, cam, prm, state, frame, md, bd, st, TH_DEPTH, rule=rule)
            stat.copy_(r["end"]["stat"], non_blocking=True)
            torch.cuda.synchronize()
    else:
        from tests import frame_step_glue as G
        from tests import frame_step_ref as R
        pin = lambda sh, dt: torch.empty(sh, dtype=dt).pin_memory()
        pinned = dict(pose=pin((1, 7), torch.float64), feat_mp=pin((1, NF), torch.int32), match_last=pin((1, NF), torch.int32),
                      match_local=pin((1, NF), torch.int32), outlier=pin((1, NF), torch.uint8), counts2=pin((1, 4), torch.int32),
                      local_mp=pin((1, NPCAP), torch.int32), n_local_mp=pin((1,), torch.int32), ref_kf=pin((1,), torch.int32))
        up = dict(last_pt=pin((1, NF, 3), torch.float64), last_valid=pin((1, NF), torch.uint8), last_observed=pin((1, NF), torch.uint8),
                  last_desc=pin((1, NF, 32), torch.uint8), last_mp=pin((1, NF), torch.int32), held=pin((1, NF), torch.uint8), pose_lw=pin((1, 7), torch.float64),
                  pose_cw=pin((1, 7), torch.float64))
        devb = {k: torch.empty_like(v, device="cuda") for k, v in up.items()}
        a = {k: frame[k] for k in frame_step.FRAME_KEYS if k != "feat_depth"}
        a.update({k: state[k] for k in frame_step.STATE_KEYS[:8]})
        lm = dict(state["lists"], last_mp=state["last_mp"])
        depth = frame["feat_depth"].cpu().numpy()

        # the host's mirror of the map, as a host that follows the map keeps it: per row "has observations" and the weighted count
        rows = np.arange(NMP)
        has_obs, weight = G.observed(m, rows), G.weighted_count(m, ba, rows)
        valid, kf_mp, mp_pos, mp_desc, kf_pose = m["mp_valid"] != 0, m["kf_mp"], m["mp_pos"], m["mp_desc"], ba["kf_pose"]
        F32 = np.float32

        def host_loop(h):
            """the loop over the features that follows the copy back, vectorised: the rules of gl_track_frame_end / gl_track_frame_next"""
            fm, ml, ol = h["feat_mp"][0], h["match_local"][0], h["outlier"][0]
            nl = min(max(int(h["n_local_mp"][0]), 0), NPCAP)
            use = (ml >= 0) & (ml < nl)
            r = np.where(use, h["local_mp"][0][np.clip(ml, 0, NPCAP - 1)], fm)
            keep = (r >= 0) & has_obs[np.maximum(r, 0)] & (ol == 0)
            in_depth = (depth[0] > 0) & (depth[0] < F32(TH_DEPTH))
            nmi, num_map, num_total = int(keep.sum()), int((keep & in_depth).sum()), int(in_depth.sum())
            ratio = F32(num_map) / F32(max(1, num_total))
            k = int(h["ref_kf"][0])
            p = kf_mp[k]
            nref = int(((p >= 0) & valid[np.maximum(p, 0)] & (weight[np.maximum(p, 0)] >= 3)).sum())
            c2 = (F32(nmi) < F32(nref) * F32(0.75) or ratio < (F32(0.2) if nmi > 300 else F32(0.35))) and nmi > 15
            need = bool(c2)  # (is_idle)
            held = np.where(keep, r, -1).astype(np.int32)
            row = held >= 0
            at = np.maximum(held, 0)
            Tkw, Tcw = R.se3_load(kf_pose[k]), R.se3_load(h["pose"][0])
            Tcr = R.se3_inverse(R.se3_mul(Tkw, R.se3_inverse(Tcw)))
            lw = R.se3_mul(Tcr, Tkw)
            return dict(last_mp=held, last_pt=np.where(row[:, None], mp_pos[at], 0.0), last_valid=row, last_observed=row, held=row,
                        last_desc=np.where(row[:, None], mp_desc[at], 0), pose_lw=lw, pose_cw=lw), need

        def call():
            out = map_stats.track_frame_with_stats(ctx, cam, prm, a, md, lm, st)
            for k, h in pinned.items():
                h.copy_(out[k] if k in out else lm[k], non_blocking=True)
            torch.cuda.synchronize()
            nxt, _ = host_loop({k: v.numpy() for k, v in pinned.items()})
            for k in up:
                up[k].numpy()[0] = nxt[k]
                devb[k].copy_(up[k], non_blocking=True)
            key_frame.create_temporal_points(ctx, cam, dict(pose=devb["pose_lw"], feat_uv=frame["feat_uv"], feat_depth=frame["feat_depth"], feat_oct=frame["feat_oct"],
                                                            held=devb["held"], last_outlier=out["outlier"], feat_desc=frame["feat_desc"]),
                                                 {k: devb[k] for k in ("last_pt", "last_observed", "last_valid", "last_desc")}, TH_DEPTH)
            torch.cuda.synchronize()
    res["host_to_host_us_median_min_max"] = wall_us(call, REPS)
    print(json.dumps(res))


if MODE == "calls":
    calls()
elif MODE in ("a", "b"):
    leg(MODE)
else:
    raise SystemExit("mode: run | calls | a | b")
