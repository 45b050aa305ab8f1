#!/usr/bin/env python3
"""Record the answers of the reference's own ORB extractor for its detection half and for the whole detect() as a data fixture:
tests/golden/golden_orb_detect_ref.npz.

Needs oracle/_ref/liborb_ref.so (oracle/Makefile builds it where the reference tree is present).  The fixture lets
tests/test_orb_detect_ref_pin.py and tests/test_gpu_orb_detect_ref.py hold the model, the declared expectations and the device to the
reference in a checkout without it.  The cases and the layout of the file: tests/orb_detect_ref_cases.py (key sets, images and levels
are regenerated from seeds and from the hand-built cases there and not stored; the file holds no pattern).  Recorded, tie-free cases only:
  fpl                       mnFeaturesPerLevel for nfeatures 0 .. 4 000
  oct, hand                 DistributeOctTree's vResultKeys of the seeded and the hand-built key sets
  cell_*_calls, cell_*_kp   the FAST calls ComputeKeyPointsOctTree made and its allKeypoints, with the callback finding nothing, answering
                            from a script, and answered by the model's FAST
  pyr, pyr_px               ComputePyramid's level sizes, steps and view offsets, and the levels' pixels
  detect_kp, _desc, _ab     detect()'s _keypoints and _descriptors, and cos / sin of each angle as the recording host's libm gave them
A list of arrays is stored as its concatenation and a `_n` array of lengths.

--ties: instead of recording, measure on dense scenes how often the declared order among equal sizes is this host's answer (DESIGN
section 2 states one such measurement; nothing asserts it).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import oracle_lib  # noqa: E402
from tests import orb_detect_dev as dev  # noqa: E402
from tests import orb_detect_ref as M  # noqa: E402
from tests import orb_detect_ref_cases as RC  # noqa: E402


def ties(ref):
    B = M.MIN_BORDER
    for nfeatures in (40, 400, 1000):
        levels_seen = tied = equal = rev = 0
        for seed in range(40, 48):
            per = M.features_per_level(nfeatures, 8)
            for l, img in enumerate(M.pyramid(dev.scene(seed, (256, 224)), 8)):
                h, w = img.shape
                args, info = ([(x - B, y - B, s) for x, y, s in M.candidates(img)[0]], B, w - B, B, h - B, per[l]), {}
                model = M.distribute(*args, info=info)
                got = [ref.distribute(*args) for _ in range(2)]
                levels_seen += 1
                if info["tie"]:
                    tied += 1
                    equal += got[0] == model
                    rev += got[0] == M.distribute(*args, mut=("tie_rev",))
                else:
                    assert got[0] == got[1] == model, (seed, nfeatures, l)
        print("nfeatures %4d: %d of %d levels tied; on the tied ones the declared order is this host's answer on %d, the reversed order on %d" %
              (nfeatures, tied, levels_seen, equal, rev))


def main():
    ref = oracle_lib.load_orb_ref()
    assert ref is not None, "oracle/_ref/liborb_ref.so missing: run make -C oracle where the reference tree is present"
    if "--ties" in sys.argv:
        return ties(ref)
    res = RC.record(ref)
    print("octree cases %d, hand-built %d, cell scenes %d, pyramids %d, detect key-points %s" %
          (len(res["oct_n"]), len(res["hand_n"]), len(res["cell_names"]), len(res["pyr_n"]), res["detect_kp_n"].tolist()))
    print("wrote", RC.PATH, os.path.getsize(RC.PATH), "bytes")


if __name__ == "__main__":
    main()
