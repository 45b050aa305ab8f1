#!/usr/bin/env python3
"""Device time of gl_update_map_points (the map-point refresh: MapPoint::computeDistinctiveDescriptors + updateNormalAndDepth) by HIP
events around single synchronised calls, after warm-up calls of the same shape:
    python tools/map_points_time.py [reps]
Shapes: (a) the fuse / processNewKeyFrame refresh, 1 200 points of 2 - 30 observations, what = 3; (b) the refresh after local BA,
5 000 points, what = 2; (c) 200 000 points of the default count distribution (synth.map_point_counts), what = 3.  Each shape is
checked once against tests/map_point_ref.py before it is timed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gmmloc_amd
from gmmloc_amd import api, synth
from tests import map_point_ref as M

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ctx = gmmloc_amd.Context(0)


def dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def shape(name, NP, what, counts, NKF, NFK, seed):
    m = synth.synth_map_points(NP, seed, NKF=NKF, NFK=NFK, counts=counts)
    n = np.diff(m["mp"]["obs_ptr"])
    init = dict(desc=np.zeros((NP, 32), np.uint8), normal=np.zeros((NP, 3)), max_dist=np.zeros(NP, np.float32),
                min_dist=np.zeros(NP, np.float32))
    kf, mp, out = dev(m["kf"]), dev(m["mp"]), dev(init)
    ref = {k: v.copy() for k, v in init.items()}
    M.update_map_points_ref(m["kf"], m["mp"], ref, what=what)
    with torch.cuda.stream(ctx.stream):
        api.update_map_points(ctx, kf, mp, out, what=what)
        torch.cuda.synchronize()
        same = all(out[k].cpu().numpy().tobytes() == ref[k].tobytes() for k in ref)
        for _ in range(10):
            api.update_map_points(ctx, kf, mp, out, what=what)
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            api.update_map_points(ctx, kf, mp, out, what=what)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
    ts = np.array(ts)
    print("%-44s NP %7d  what %d  observations %8d (mean %.1f, max %d)  device us: median %8.1f  min %8.1f  max %8.1f  "
          "(%d calls)  bit-equal to the restatement: %s" % (name, NP, what, int(n.sum()), n.mean(), n.max(), np.median(ts), ts.min(),
                                                           ts.max(), REPS, same))
    assert same, name


def main():
    print("gl_update_map_points, device time by HIP events around single synchronised calls, after 11 warm-up calls; %s"
          % torch.cuda.get_device_name(0))
    rng = np.random.default_rng(1)
    shape("(a) fuse / processNewKeyFrame, 2 - 30 obs", 1200, 3, rng.integers(2, 31, 1200), 257, 1000, 21)
    shape("(b) after local BA", 5000, 2, None, 257, 1000, 22)
    shape("(c) 200 000 points", 200000, 3, None, 2503, 1000, 23)


if __name__ == "__main__":
    main()
