#!/usr/bin/env python3
"""Device time of gl_orb_pyramid, gl_orb_detect and the composite orb.extract, calls enqueued back to back between two HIP events on a
warmed context's stream (as tools/orb_time.py does for gl_orb_describe): one stereo frame (B = 2, 752 x 480, eight levels) with
nfeatures 1 000 and 2 000, the latter also with 6 400 candidate slots (at 8 192 its octree's working set, 4 B per slot + 72 B per node, is
above the 56 KB it may hold in LDS and lies in the scratch block; at 6 400 it fits), and 64 such frames in one call - one process per leg.
    python tools/orb_detect_time.py [label] [--out FILE]
Writes profiles/r22_orb_detect_time.txt (or FILE) and adds the file's line to profiles/README.md when it has none.  The images are
those of tests/orb_detect_dev.py (block noise: about 6 000 candidates on level 0, about 29 000 over an image's eight levels).  There is no parent to compare against and no OpenCV
at hand: no speed-up over the reference is claimed, and the HOST time the calls save is not measured."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZE, LEVELS = (752, 480), 8
LEGS = ((1, 1000, 8192), (1, 2000, 8192), (1, 2000, 6400), (64, 1000, 8192))  # frames, nfeatures, cand_cap
DESCRIBE_US, STEREO_US = 24.4, 178.6  # profiles/r21_orb_time.txt, profiles/r20_stereo_time.txt: one such frame


def leg(label, frames, nfeatures, CAP):
    import numpy as np
    import torch

    import gmmloc_amd
    from gmmloc_amd import orb
    from tests import orb_detect_dev, orb_scenes
    ctx = gmmloc_amd.Context(0)
    dev = torch.device("cuda:0")

    def ev_us(fn, n):
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

    B = 2 * frames
    images = [orb_detect_dev.scene(11 + b, SIZE, grain=10) for b in range(4)]
    im = torch.from_numpy(np.stack([images[b % 4] for b in range(B)])).to(dev)
    pattern = torch.from_numpy(orb_scenes.PATTERN).to(dev)
    pyr = orb.build_pyramid(ctx, im, LEVELS)
    det = orb.detect(ctx, pyr, nfeatures, cand_cap=CAP)
    des = orb.describe(ctx, det["kp_xy"], det["kp_oct"], pattern, pyr, n_kp=det["n_kp"])
    torch.cuda.synchronize()
    stat = det["stat"].cpu().numpy()
    reps = 100 if frames == 1 else 10
    c = pyr.c

    def three(fn):
        return [ev_us(fn, reps) for _ in range(3)]

    t_pyr = three(lambda: ctx.call(ctx.lib.gl_orb_pyramid, B, c, 1.2))
    t_det = three(lambda: orb.detect(ctx, pyr, nfeatures, cand_cap=CAP, out=det))
    t_all = three(lambda: (ctx.call(ctx.lib.gl_orb_pyramid, B, c, 1.2), orb.detect(ctx, pyr, nfeatures, cand_cap=CAP, out=det),
                           orb.describe(ctx, det["kp_xy"], det["kp_oct"], pattern, pyr, n_kp=det["n_kp"], out=des)))
    fmt = lambda us: " ".join("%.1f" % u for u in us)
    print("%s: B = %3d (%2d frame%s x 2 sides, %d x %d, %d levels, nfeatures %d, cand_cap %d): gl_orb_pyramid %s | gl_orb_detect %s | pyramid + "
          "detect + describe %s us per call (three runs each); per frame %.1f | %.1f | %.1f us; image 0: %d candidates, %d cells redone, %d "
          "key-points, overflow mask %d" % (label, B, frames, "s" if frames > 1 else " ", SIZE[0], SIZE[1], LEVELS, nfeatures, CAP, fmt(t_pyr),
                                            fmt(t_det), fmt(t_all), min(t_pyr) / frames, min(t_det) / frames, min(t_all) / frames, *stat[0]))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--leg":
        leg(args[1], int(args[2]), int(args[3]), int(args[4]))
        sys.exit(0)
    out_path = os.path.join(ROOT, "profiles", "r22_orb_detect_time.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
        del args[args.index("--out"):args.index("--out") + 2]
    label = args[0] if args else "lib"
    lines = ["# python tools/orb_detect_time.py %s   (one MI355X; libgmmloc_hip.so built from this tree; one process per leg)" % label]
    for frames, nfeatures, cap in LEGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", label, str(frames), str(nfeatures), str(cap)], capture_output=True, text=True,
                           timeout=200)
        if r.returncode != 0:  # a leg that failed ends the run: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode or 1)
        lines.append(r.stdout.strip())
    lines.append("# beside gl_orb_describe: %.1f us and gl_stereo_matches: %.1f us for one such frame (profiles/r21_orb_time.txt, r20_stereo_time.txt).  "
                 "No parent and no OpenCV to compare against: no speed-up over the reference is claimed; the host time saved (fourteen resizes, "
                 "FAST on sixteen levels, the octrees and the upload of pyramids and key-points) is unmeasured." % (DESCRIBE_US, STEREO_US))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as fh:
        fh.write(text)
    index = os.path.join(ROOT, "profiles", "README.md")
    name = os.path.basename(out_path)
    if os.path.exists(index) and name not in open(index).read():
        row = ("| `%s` | `tools/orb_detect_time.py`: device time of `gl_orb_pyramid`, `gl_orb_detect` and the three-call composite by HIP events "
               "around back-to-back calls on a warmed context, one process per leg - one stereo frame (B = 2, 752 x 480, eight levels) at "
               "nfeatures 1 000 and 2 000 (the latter with the octree's working set in the scratch block and in LDS), and 64 such frames; no "
               "speed-up over the reference is claimed and the host time saved is unmeasured |" % name)
        rows = open(index).read().split("\n")
        last = max(i for i, l in enumerate(rows) if l.startswith("| `"))  # behind the table's last row
        rows.insert(last + 1, row)
        with open(index, "w") as fh:
            fh.write("\n".join(rows))
