#!/usr/bin/env python3
"""Device time of gl_orb_describe, calls enqueued back to back between two HIP events on a warmed context's stream (as
tools/stereo_time.py does for gl_stereo_matches): one stereo frame's two sides as one call (B = 2, 1 200 key-points each on a 752 x 480
eight-level pyramid), and 64 such frames (B = 128); the same calls with ONE key-point per image, which is the blur and an empty describe
launch, for the blur's achieved bytes per second against the pyramid's read + write size.
    python tools/orb_time.py [label] [--out FILE]
Writes profiles/r21_orb_time.txt (or FILE) and adds the file's line to profiles/README.md when it has none.  The scenes are those of
tests/orb_scenes.py (textured levels, a seeded synthetic pattern).  There is no parent to compare against and no OpenCV at hand: no
speed-up over the reference is claimed, and the HOST time the call saves is not measured."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gmmloc_amd
from gmmloc_amd import orb, stereo
from tests import orb_scenes

args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "r21_orb_time.txt")
if "--out" in args:
    out_path = args[args.index("--out") + 1]
    del args[args.index("--out"):args.index("--out") + 2]
label = args[0] if args else "lib"
ctx = gmmloc_amd.Context(0)
N, SIZE, LEVELS = 1200, (752, 480), 8
STEREO_US = 178.6  # gl_stereo_matches for one such frame (profiles/r20_stereo_time.txt)


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


lines = ["# python tools/orb_time.py %s   (one MI355X; libgmmloc_hip.so built from this tree)" % label]
scenes = [orb_scenes.random_scene(900 + b, size=SIZE, nlevels=LEVELS, n=N, stray_every=10 ** 9) for b in range(4)]
dev = torch.device("cuda:0")
pattern = torch.from_numpy(scenes[0]["pattern"]).to(dev)
pyramid_bytes = sum(im.size for im in scenes[0]["levels"])
for frames in (1, 64):
    B = 2 * frames
    pick = [scenes[b % len(scenes)] for b in range(B)]
    pyr = stereo.Pyramid([s["levels"] for s in pick], dev)
    xy = torch.from_numpy(np.stack([s["kp_xy"] for s in pick])).to(dev)
    oct_ = torch.from_numpy(np.stack([s["kp_oct"] for s in pick])).to(dev)
    out = orb.describe(ctx, xy, oct_, pattern, pyr)
    torch.cuda.synchronize()
    stat = out["stat"].cpu().numpy()
    reps = 200 if frames == 1 else 30
    us = [ev_us(lambda: orb.describe(ctx, xy, oct_, pattern, pyr, out=out), reps) for _ in range(3)]
    xy1, oct1 = xy[:, :1].contiguous(), oct_[:, :1].contiguous()
    out1 = orb.describe(ctx, xy1, oct1, pattern, pyr)
    us1 = [ev_us(lambda: orb.describe(ctx, xy1, oct1, pattern, pyr, out=out1), reps) for _ in range(3)]
    moved = 2 * B * pyramid_bytes
    lines.append("%s: B = %3d (%2d frame%s x 2 sides x %d key-points, %d x %d, %d levels): %s us per call (three runs), %.1f us per frame; "
                 "image 0: %d described, %d skipped" % (label, B, frames, "s" if frames > 1 else " ", N, SIZE[0], SIZE[1], LEVELS,
                                                         " ".join("%.1f" % u for u in us), min(us) / frames, stat[0, 0], stat[0, 1]))
    lines.append("%s: B = %3d, one key-point per image (the blur + an empty describe launch): %s us per call; the pyramids' read + write size "
                 "%.2f MB -> %.1f GB/s" % (label, B, " ".join("%.1f" % u for u in us1), moved / 1e6, moved / (min(us1) * 1e-6) / 1e9))
lines.append("# beside gl_stereo_matches: %.1f us for one such frame (profiles/r20_stereo_time.txt).  No parent and no OpenCV to compare against: "
             "no speed-up over the reference is claimed; the host time saved (sixteen level blurs and 2 x 1 200 descriptors) is unmeasured." % STEREO_US)
text = "\n".join(lines) + "\n"
print(text, end="")
with open(out_path, "w") as fh:
    fh.write(text)
index = os.path.join(ROOT, "profiles", "README.md")
name = os.path.basename(out_path)
if os.path.exists(index) and name not in open(index).read():
    with open(index, "a") as fh:
        fh.write("| `%s` | `tools/orb_time.py`: device time of `gl_orb_describe` by HIP events around back-to-back calls on a warmed context - one "
                 "stereo frame's two sides (B = 2 x 1 200 key-points, 752 x 480, eight levels) and 64 such frames - and the blur's achieved "
                 "bytes per second, with the run's command and the library's commit |\n" % name)
