"""tools/record_ba_bits.py OUT.json: run the cases of tests/test_gpu_ba_bits.py on cuda:0 and write their sha256 (poses, points,
dropped, erase[:nobs], iters) - to be run on the commit whose bits are to be kept (GMMLOC_HIP_LIB selects a library built from
it), the result committed as tests/golden/ba_bits_parent.json."""
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
    from tests import test_gpu_ba_bits as T
    d = np.load(os.path.join(ROOT, "tests", "golden", "map_v1.npz"))
    ctx = gmmloc_amd.Context(0)
    g = api.GMM(ctx, d["mean"], d["cov"])
    sha = {}
    for cid in T.all_cases():
        for shape in sorted(T.SHAPES):
            key = T.case_id(cid, shape)
            sha[key] = T.digest(T.run_case(torch, ctx, g, cid, shape))
            print(key, sha[key], flush=True)
    with open(out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "sha256": sha}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
