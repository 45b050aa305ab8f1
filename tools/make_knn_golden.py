#!/usr/bin/env python3
"""Record the reference's own nanoflann k-NN answers as a data fixture: tests/golden/golden_nanoflann_knn.npz.

Needs oracle/_ref/libnanoflann_ref.so (oracle/Makefile builds it where the reference tree is present).  The
fixture lets tests/test_oracle_golden.py and tests/test_gpu_gmm_assoc.py check the kNN stages against nanoflann
in a checkout without the reference:
  v1_pts, v2_pts          800 x 3 queries (synth.synth_points(map, 800, 3)) on the two maps
  v{1,2}_idx/_dist/_cnt   nanoflann's 5-NN over the map means for them
  v{1,2}_gpu_idx          nanoflann's 5-NN for the 1500 queries of test_knn3d_and_query_point (synth_points(map, 1500, 9))
  few_*, q2d_*            a 3-point 2-D tree queried by 10 points with k = 5 (fewer points than k)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gmmloc_amd import synth  # noqa: E402
from tests import oracle_lib  # noqa: E402


def main():
    orc = oracle_lib.load()
    assert orc.nf is not None, "oracle/_ref/libnanoflann_ref.so missing: run make -C oracle where the reference tree is present"
    out = {}
    for name in ("v1", "v2"):
        d = np.load(os.path.join(ROOT, "tests", "golden", "map_%s.npz" % name))
        mean, cov = d["mean"], d["cov"]
        pts = synth.synth_points(mean, cov, 800, 3)
        out[name + "_pts"] = pts
        out[name + "_idx"], out[name + "_dist"], out[name + "_cnt"] = orc.nanoflann_knn(mean, pts, 5)
        out[name + "_gpu_idx"] = orc.nanoflann_knn(mean, synth.synth_points(mean, cov, 1500, 9), 5)[0]
    few = np.random.default_rng(0).uniform(0, 100, (3, 2))
    q = np.random.default_rng(1).uniform(0, 100, (10, 2))
    out["few_pts"], out["q2d"] = few, q
    out["q2d_idx"], out["q2d_dist"], out["q2d_cnt"] = orc.nanoflann_knn(few, q, 5)
    path = os.path.join(ROOT, "tests", "golden", "golden_nanoflann_knn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
