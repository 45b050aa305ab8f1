#!/usr/bin/env python3
"""Record the answers of the reference's own ORB extractor as a data fixture: tests/golden/golden_orb_ref.npz.

Needs oracle/_ref/liborb_ref.so (oracle/Makefile builds it where the reference tree is present).  The fixture lets
tests/test_orb_ref_pin.py and tests/test_gpu_orb_ref.py hold the model, the declared expectations and the device to the reference in a
checkout without it.  The cases and the layout of the file: tests/orb_ref_cases.py (images, key-points and patterns are regenerated
from the hand-built cases and from seeds there and not stored; the file holds no pattern).  Per described key-point:
  angle_bits, m_10, m_01   computeOrientation's angle and the moments it handed to fastAtan2
  ab_bits                  cos / sin of the steering angle as the recording host's libm gave them to computeOrbDescriptor
  desc                     computeDescriptors' 32 bytes
and the tables umax and mvScaleFactor of a constructed extractor.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import oracle_lib  # noqa: E402
from tests import orb_ref_cases as RC  # noqa: E402


def main():
    ref = oracle_lib.load_orb_ref()
    assert ref is not None, "oracle/_ref/liborb_ref.so missing: run make -C oracle where the reference tree is present"
    results, tables = RC.record(ref)
    n = sum(len(r["angle"]) for r in results.values())
    off = sum(int((~RC.declared_steering(RC.cases()[name], r)).sum()) for name, r in results.items())
    print("cases %d, key-points %d, of them %d steered by an (a, b) other than the correctly rounded one" % (len(results), n, off))
    print("umax", tables["umax"].tolist(), "scale factors", tables["scale_factor"].tolist())
    print("wrote", RC.PATH, os.path.getsize(RC.PATH), "bytes")


if __name__ == "__main__":
    main()
