#!/usr/bin/env python3
"""The three measurements of DESIGN.md section 2 on the reference's ORB extractor as built on THIS host (oracle/_ref/liborb_ref.so and
liborb_ref_contract.so): statements about the reference under this compiler and libm, not thresholds - nothing asserts them.
  1. steering: the share of the angles k x 1e-5 degrees, k = 0 .. 36 000 000, at which the host's float cos / sin differ from the declared
     steering (float)cos((double)rad) / (float)sin((double)rad)
  2. descriptors under libm steering: on random scenes (tests/orb_ref_cases.py's geometry), the share of key-points and of descriptor
     bits that differ between the model under the declared steering and the reference
  3. contraction: the same two shares between the -ffp-contract=off build and the -O3 -mfma -ffp-contract=fast build
"""
import os
import platform
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import oracle_lib, orb_ref  # noqa: E402
from tests import orb_ref_cases as RC  # noqa: E402

POPCOUNT = np.array([bin(i).count("1") for i in range(256)])


def shares(a, b):
    d = POPCOUNT[a ^ b]
    return "%d of %d key-points (%.2f %%), %d of %d bits (%.4f %%)" % ((d.sum(1) > 0).sum(), len(d), 100.0 * (d.sum(1) > 0).mean(), d.sum(), d.size * 8,
                                                                       100.0 * d.sum() / (d.size * 8))


def main(nscenes=100):
    ref, con = oracle_lib.load_orb_ref(), oracle_lib.load_orb_ref(contract=True)
    assert ref is not None and con is not None, "make -C oracle where the reference tree is present"
    print("host:", subprocess.check_output(["g++", "--version"]).decode().splitlines()[0], "|", " ".join(platform.libc_ver()))
    n = bad_a = bad_b = bad = far = 0
    for k0 in range(0, 36000001, 4000000):
        k = np.arange(k0, min(k0 + 4000000, 36000001), dtype=np.float64)
        ang = (k * 1e-5).astype(np.float32)
        rad = (ang * orb_ref.FACTOR_PI).astype(np.float64)
        ab = ref.steering(ang)
        want = np.stack([np.cos(rad), np.sin(rad)], 1).astype(np.float32)
        da, db = ab[:, 0] != want[:, 0], ab[:, 1] != want[:, 1]
        far += int(((ab != want) & (ab != np.nextafter(want, np.float32(2))) & (ab != np.nextafter(want, np.float32(-2)))).sum())
        n, bad_a, bad_b, bad = n + len(k), bad_a + int(da.sum()), bad_b + int(db.sum()), bad + int((da | db).sum())
    print("steering: cos differs at %d, sin at %d of %d angles (%.3f %%, %.3f %%); a or b at %d (%.3f %%); further than the neighbouring float: %d" %
          (bad_a, bad_b, n, 100.0 * bad_a / n, 100.0 * bad_b / n, bad, 100.0 * bad / n, far))
    declared, libm, fused = [], [], []
    for i in range(nscenes):
        c = RC.scene("given" if i % 2 else "computed", seed=7100 + i)
        s = RC.slots(c)
        declared.append(orb_ref.describe(**RC.model_args(c))["desc"][s])
        libm.append(RC.live_case(ref, c)["desc"])
        fused.append(RC.live_case(con, c)["desc"])
    declared, libm, fused = (np.concatenate(x) for x in (declared, libm, fused))
    print("descriptors, declared against libm steering, %d scenes: %s" % (nscenes, shares(declared, libm)))
    print("descriptors, -ffp-contract=off against -O3 -mfma -ffp-contract=fast, %d scenes: %s" % (nscenes, shares(libm, fused)))


if __name__ == "__main__":
    main()
