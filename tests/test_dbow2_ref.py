"""The vocabulary transform and its reader against the reference's OWN DBoW2 code, on the CPU: what oracle/_ref/libdbow2_ref.so gave
(TemplatedVocabulary<FORB::TDescriptor, FORB> compiled where it lies, oracle/dbow2_ref.cpp), as recorded in tests/golden/
golden_dbow2_ref.npz, holds the restatement tests/bow_ref.py, the declared expectations of tests/bow_cases.py and gl_voc_file_read,
every comparison exact.  The tests on the recorded file never skip; where the library is built it is run as well and must reproduce
the file.  Declared deviations (1) the phantom and (3) the shallow leaf of DESIGN row 8f-6 are tested facts here.  The device:
tests/test_gpu_dbow2_ref.py."""
import functools

import numpy as np
import pytest

from gmmloc_amd import synth
from tests import bow_cases as BC
from tests import bow_ref as R
from tests import dbow2_cases as DC
from tests import oracle_lib

NAMES = list(DC.cases())


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def tree(name):
    return R.Tree(DC.cases()[name]["voc"])


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """every case through the live library, once; skips where it is not built"""
    ref = oracle_lib.load_dbow2()
    if ref is None:
        pytest.skip("oracle/_ref/libdbow2_ref.so not built")
    return DC.live(ref, tmp_path_factory.mktemp("dbow2_ref"))


def in_slots(c, r):
    """a recorded result in the slots of the case: (word, node, weight, fv) as bow_ref.transform gives them"""
    o = DC.as_outputs(c, r)
    s = DC.slots(c)
    return o["word_id"][0], o["node"][0], o["weight"][0], [(n, [int(s[i]) for i in f]) for n, f in r["fv"]]


def test_the_file_holds_every_case():
    rec, dump = DC.recorded()
    assert list(rec) == NAMES
    for name, c in DC.cases().items():
        r = rec[name]
        n = len(DC.slots(c))
        assert len(r["word"]) == len(r["weight"]) == len(r["nid"]) == len(r["final"]) == n and r["levelsup"] == c["levelsup"], name
        kept = sorted(i for _, f in r["fv"] for i in f)
        assert kept == np.nonzero(r["weight"] > 0)[0].tolist(), name  # the features with weight > 0, each once
        assert [n for n, _ in r["fv"]] == sorted(set(n for n, _ in r["fv"])) and all(f == sorted(f) for _, f in r["fv"]), name
        assert r["overload"] == (not (r["nid"] == DC.NID_UNSET).any()), name


# ---- the restatement and the declared expectations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(name):
    """bow_ref.transform == the reference in word ids, weight bits, node ids and the feature vector; where the reference left nid
    unwritten the expected node is the final node the reference itself reports: no feature is left out"""
    c, r = DC.cases()[name], DC.recorded()[0][name]
    word, node, weight, fv = R.transform(tree(name), c["desc"], c["oct"], c["levelsup"])
    rw, rn, rwt, rfv = in_slots(c, r)
    assert bits_equal(word, rw) and bits_equal(node, rn) and bits_equal(weight, rwt)
    assert [(int(n), [int(i) for i in f]) for n, f in fv] == rfv


@pytest.mark.parametrize("name", list(BC.CASES))
def test_declared_expectations_equal_the_reference(name):
    c, e, r = DC.cases()["case/" + name], BC.CASES[name]["expect"], DC.recorded()[0]["case/" + name]
    rw, rn, rwt, rfv = in_slots(c, r)
    assert bits_equal(e["word_id"], rw) and bits_equal(e["node"], rn) and bits_equal(e["weight"], rwt)
    assert e["fv"] == rfv


# ---- deviation (1): the phantom ---------------------------------------------------------------------------------------------------------------
def test_the_reference_appends_a_phantom_that_no_feature_reaches():
    rec, dump = DC.recorded()
    v = DC.dump_voc()
    n = len(v["parent"])  # records; the header's nb_nodes is n + 1
    flagged = int((v["is_leaf"] != 0).sum())
    assert dump["info"].tolist() == [n + 2, flagged + 1, v["k"], v["L"]]  # nb_nodes + 1 nodes, one word more than the file flags
    ph = n + 1
    last_parent = int(v["parent"][-1])
    assert dump["parent"][ph] == last_parent
    assert dump["child_ids"][dump["child_ptr"][last_parent]:dump["child_ptr"][last_parent + 1]].tolist()[-2:] == [n, ph]  # the last child, behind the last record
    assert bits_equal(dump["desc"][ph], v["desc"][-1]) and bits_equal(dump["weight"][ph], v["weight"][-1])
    assert dump["word_id"][ph] == flagged and dump["child_ptr"][ph] == dump["child_ptr"][ph + 1]
    for name, c in DC.cases().items():  # the same counts on every vocabulary; no feature ends on the phantom
        r, nrec, nflag = rec[name], len(c["voc"]["parent"]), int((np.asarray(c["voc"]["is_leaf"]) != 0).sum())
        assert (r["voc_nodes"], r["voc_words"]) == (nrec + 2, nflag + 1), name
        assert (r["final"] <= nrec).all() and (r["final"] >= 1).all() and (r["word"] < nflag).all() and (r["word"] >= 0).all(), name


def test_the_strict_compare_keeps_the_phantom_out():
    """last_record_nearest: the last record is the unique nearest child at distance 0, the phantom behind it holds the same bytes"""
    c, r = BC.CASES["last_record_nearest"], DC.recorded()[0]["case/last_record_nearest"]
    d = np.array([[R.POPCOUNT[f ^ ch].sum() for ch in c["voc"]["desc"]] for f in c["desc"]])
    assert d[0].tolist() == [14, 14, 14, 14, 0] and d[1, 4] == d[1].min() and (d[1] == d[1].min()).sum() == 1
    assert r["word"].tolist() == [4, 4, 3] and r["final"].tolist() == [5, 5, 4] and r["voc_nodes"] == 7 and r["voc_words"] == 6


# ---- deviation (3): the shallow leaf --------------------------------------------------------------------------------------------------------
def test_nid_is_left_unwritten_exactly_on_shallow_leaves():
    """the reference leaves nid unwritten exactly where the restatement takes its `nid is None` branch, and nowhere else"""
    rec = DC.recorded()[0]
    count = {}
    for name, c in DC.cases().items():
        t = tree(name)
        mine = np.array([t.descend(np.asarray(f, np.uint8), c["levelsup"])[1] is None for f in c["desc"][DC.slots(c)]], bool).reshape(-1)
        theirs = rec[name]["nid"] == DC.NID_UNSET
        assert np.array_equal(mine, theirs), name
        count[name] = int(theirs.sum())
    print("nid left unwritten:", {k: v for k, v in count.items() if v}, "in all", sum(count.values()))
    assert count["case/shallow_leaf"] == 2 and count["case/shallow_leaf_levelsup_1"] == 1
    for voc in ("k10_L4_early", "k3_L6_early"):
        assert count["synth/%s/levelsup_0" % voc] > 0 and count["synth/%s/levelsup_%d" % (voc, DC.SYNTH[voc][1] + 3)] == 0
    assert all(v == 0 for k, v in count.items() if k.split("/")[1] in ("k10_L4", "k3_L6"))
    assert all(v == 0 for k, v in count.items() if k.startswith("case/") and "shallow_leaf" not in k)


# ---- the reader -----------------------------------------------------------------------------------------------------------------------------------
def test_reader_equals_the_reference_node_dump_less_the_phantom(tmp_path):
    """gl_voc_file_read (host only) on the interleaved vocabulary: its arrays == the reference's m_nodes without the root and the
    phantom; the leaf flag == children.empty(); word ids in flag order"""
    from gmmloc_amd import bow
    dump = DC.recorded()[1]
    v = DC.dump_voc()
    p = tmp_path / "voc.bin"
    synth.write_vocabulary_file(p, v)
    got = bow.read_vocabulary_file(p)
    n = len(got["parent"])
    assert n + 2 == dump["info"][0] and (got["k"], got["L"]) == (dump["info"][2], dump["info"][3])
    assert bits_equal(got["parent"], dump["parent"][1:n + 1]) and bits_equal(got["desc"], dump["desc"][1:n + 1])
    assert bits_equal(got["weight"], dump["weight"][1:n + 1])
    assert np.isnan(got["weight"][0]) and np.signbit(got["weight"][1]) and got["weight"][2] == BC.F32_DENORM_MIN  # (the special weights went through)
    nchild = np.diff(dump["child_ptr"])[1:n + 1]
    assert np.array_equal(got["is_leaf"] != 0, nchild == 0)
    assert np.array_equal(np.where(got["is_leaf"] != 0, np.cumsum(got["is_leaf"] != 0) - 1, -1), dump["word_id"][1:n + 1])
    assert dump["word_id"][0] == -1 and dump["child_ptr"][0] == 0
    # the children of every node in stored order = ascending id (the loader's push_back order), as the restatement's Tree lists them
    t = R.Tree(got)
    for nid in range(n + 1):
        ref_children = [int(x) for x in dump["child_ids"][dump["child_ptr"][nid]:dump["child_ptr"][nid + 1]] if x <= n]
        assert t.children(nid).tolist() == ref_children, nid
    assert len(set(np.diff(dump["child_ids"][:-1]).tolist())) > 1  # interleaved: the children of one node are not consecutive ids


# ---- the live library -------------------------------------------------------------------------------------------------------------------------
def test_live_library_reproduces_the_file(live):
    results, dump, overload_fv = live
    packed, stored = DC.pack(results, dump), np.load(DC.PATH)
    assert sorted(packed) == sorted(stored.files)
    for k in packed:
        assert bits_equal(packed[k], stored[k]), k
    ran = [n for n in results if overload_fv[n] is not None]
    assert ran == [n for n in results if not (results[n]["nid"] == DC.NID_UNSET).any()] and len(ran) > 30
    for n in ran:  # the vector overload transform(features, bv, fv, levelsup) == addFeature on the per-feature results
        assert overload_fv[n] == results[n]["fv"], n


def test_live_distance_equals_the_restatement():
    """FORB::distance == bow_ref's distance at 0, 1, 128, 255, 256 and on one descriptor per single bit"""
    ref = oracle_lib.load_dbow2()
    if ref is None:
        pytest.skip("oracle/_ref/libdbow2_ref.so not built")
    zero = BC.bits()
    pairs = [(zero, zero, 0), (BC.ONES, BC.ONES, 0), (zero, BC.bits(77), 1), (zero, BC.bits(*range(0, 256, 2)), 128),
             (BC.bits(*range(64, 192)), BC.bits(*range(128, 256)), 128), (BC.ONES, BC.bits(200), 255), (zero, BC.bits(*range(1, 256)), 255),
             (zero, BC.ONES, 256)]
    pairs += [(BC.bits(b), zero, 1) for b in range(256)] + [(BC.bits(b), BC.bits((b + 1) % 256), 2) for b in range(256)]
    for a, b, want in pairs:
        t = R.Tree(BC.voc([0], [b]))
        assert ref.distance(a, b) == ref.distance(b, a) == t.distance(a, 1) == want
