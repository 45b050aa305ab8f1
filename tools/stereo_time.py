#!/usr/bin/env python3
"""Device time of gl_stereo_matches, calls enqueued back to back between two HIP events on a warmed context's stream (as
tools/chain_ab.py does for the chain): one frame of 1 200 + 1 200 key-points on a 752 x 480 eight-level pyramid, and 64 such frames.
    python tools/stereo_time.py [label]
The scenes are those of tests/stereo_scenes.py (textured levels, the right one shifted, partner descriptors), so the work per feature is
that of a frame whose features mostly match."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gmmloc_amd
from gmmloc_amd import api, stereo
from tests import stereo_scenes

label = sys.argv[1] if len(sys.argv) > 1 else "lib"
ctx = gmmloc_amd.Context(0)
NF, SIZE, LEVELS = 1200, (752, 480), 8


def ev_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(ctx.stream):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        e0.record(ctx.stream)
        for _ in range(n):
            fn()
        e1.record(ctx.stream)
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


scenes = [stereo_scenes.random_scene(900 + b, size=SIZE, nlevels=LEVELS, nfeat=NF) for b in range(4)]
fx, bf, height = scenes[0]["cam"]
cam = api.Camera(fx=fx, fy=fx, bf=bf, height=height)
dev = torch.device("cuda:0")
for B in (1, 64):
    frames = [scenes[b % len(scenes)]["frame"] for b in range(B)]
    t = {k: torch.from_numpy(np.stack([f[k] for f in frames])).to(dev) for k in ("feat_uv", "feat_oct", "feat_desc", "r_uv", "r_oct", "r_desc")}
    pl = stereo.Pyramid([f["pyr_left"] for f in frames], dev)
    pr = stereo.Pyramid([f["pyr_right"] for f in frames], dev)
    left, right = {k: t[k] for k in ("feat_uv", "feat_oct", "feat_desc")}, {k: t[k] for k in ("r_uv", "r_oct", "r_desc")}
    out = stereo.stereo_matches(ctx, cam, left, right, pl, pr)
    torch.cuda.synchronize()
    stat = out["stat"].cpu().numpy()
    us = [ev_us(lambda: stereo.stereo_matches(ctx, cam, left, right, pl, pr, out=out), 200 if B == 1 else 50) for _ in range(3)]
    print("%s: B = %2d x (%d + %d key-points, %d x %d, %d levels): %s us per call (three runs), %.1f us per frame; frame 0: %d pass :261, %d matched, %d reset"
          % (label, B, NF, NF, SIZE[0], SIZE[1], LEVELS, " ".join("%.1f" % u for u in us), min(us) / B, stat[0, 0], stat[0, 1], stat[0, 2]))
