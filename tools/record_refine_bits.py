"""tools/record_refine_bits.py OUT.json: run the cases of tests/test_gpu_refine_bits.py on cuda:0 and write their sha256
(pose, points, associations) - to be run on the commit whose bits are to be kept, the result committed as
tests/golden/refine_bits_parent.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    import torch
    import gmmloc_amd
    from gmmloc_amd import api
    from tests import test_gpu_refine_bits as T
    golden = os.path.join(ROOT, "tests", "golden")
    d = np.load(os.path.join(golden, "map_v1.npz"))
    map_v1 = (d["mean"], d["cov"])
    gt_sync = np.load(os.path.join(golden, "gt_sync.npz"))
    ctx = gmmloc_amd.Context(0)
    g = api.GMM(ctx, *map_v1)
    sha = {}
    for M, B, anchored in T.all_case_params():
        frames = T.build_frames(map_v1, gt_sync, M, B)
        res = {s: T.run_case(torch, ctx, g, frames, s, anchored) for s in (0, 1)}
        for a, b, what in zip(res[0], res[1], T.WHAT):
            assert np.array_equal(a, b, equal_nan=True), ("DENSE != SPREAD", M, B, anchored, what)
        for s in (0, 1):
            sha[T.case_id(M, B, s, anchored)] = T.digest(res[s])
            print(T.case_id(M, B, s, anchored), sha[T.case_id(M, B, s, anchored)], flush=True)
    with open(out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "sha256": sha}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
