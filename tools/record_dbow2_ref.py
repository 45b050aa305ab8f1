#!/usr/bin/env python3
"""Record the answers of the reference's own DBoW2 as a data fixture: tests/golden/golden_dbow2_ref.npz.

Needs oracle/_ref/libdbow2_ref.so (oracle/Makefile builds it where the reference tree is present).  The fixture lets
tests/test_dbow2_ref.py and tests/test_gpu_dbow2_ref.py hold the restatement, the declared expectations and the device to the
reference in a checkout without it.  The cases and the layout of the file: tests/dbow2_cases.py (vocabularies and descriptors are
regenerated from seeds there and not stored).  Per case, in the reference's own feature indices:
  word, weight_bits, nid, final   the per-feature transform; nid = 0xFFFFFFFF where the reference left it unwritten
  node_id / node_cnt / node_idx   the feature vector by FeatureVector::addFeature, in map order
  overload                        the vector overload transform(features, bv, fv, levelsup) was run and gave that same vector
  dump_*                          the reference's m_nodes after loading the small interleaved vocabulary, the phantom included
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dbow2_cases as DC  # noqa: E402
from tests import oracle_lib  # noqa: E402


def main():
    ref = oracle_lib.load_dbow2()
    assert ref is not None, "oracle/_ref/libdbow2_ref.so missing: run make -C oracle where the reference tree is present"
    with tempfile.TemporaryDirectory() as tmp:
        results, dump, overload_fv = DC.live(ref, tmp)
    for name, r in results.items():
        assert overload_fv[name] is None or overload_fv[name] == r["fv"], name  # the two routes to the feature vector agree
    unwritten = {n: int((r["nid"] == DC.NID_UNSET).sum()) for n, r in results.items()}
    for n, u in unwritten.items():
        if u:
            print("%-40s nid left unwritten for %d of %d features" % (n, u, len(results[n]["nid"])))
    print("cases %d, features %d, nid left unwritten %d, vector overload run on %d cases" %
          (len(results), sum(len(r["word"]) for r in results.values()), sum(unwritten.values()), sum(r["overload"] for r in results.values())))
    print("node dump: %d nodes, %d words (k %d, L %d)" % tuple(dump["info"]))
    np.savez_compressed(DC.PATH, **DC.pack(results, dump))
    print("wrote", DC.PATH, os.path.getsize(DC.PATH), "bytes")


if __name__ == "__main__":
    main()
