"""gl_voc_create / gl_voc_load_file / gl_bow_transform on the device against the reference's OWN DBoW2 code, exactly: what
oracle/_ref/libdbow2_ref.so gave for the cases of tests/dbow2_cases.py, as recorded in tests/golden/golden_dbow2_ref.npz (the
reference tree itself is never read here), and the live library as well where it has been built.  Word, node and weight bits per
feature and the feature vector as CSR on sentinel-filled buffers; the reference's compacted feature indices are mapped back to slots
(padding is this project's notion), and where the reference left nid unwritten the node is the final node it reports itself."""
import numpy as np
import pytest

from gmmloc_amd import synth
from tests import dbow2_cases as DC
from tests import oracle_lib
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (autouse fixture)
from tests.test_gpu_bow_cases import FILL, T, device_transform, device_voc, same

pytestmark = pytest.mark.gpu
NAMES = list(DC.cases())
_dev = {}


def dev_voc(ctx, c):
    """one device vocabulary per host vocabulary, made once"""
    if id(c["voc"]) not in _dev:
        _dev[id(c["voc"])] = device_voc(ctx, c["voc"])
    return _dev[id(c["voc"])]


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """{name: result} of the live library where oracle/_ref/libdbow2_ref.so is present, else None"""
    ref = oracle_lib.load_dbow2()
    return None if ref is None else DC.live(ref, tmp_path_factory.mktemp("dbow2_ref"))[0]


def references(name, live):
    return [("recorded", DC.recorded()[0][name])] + ([("live", live[name])] if live is not None else [])


def octaves(c):
    return None if c["oct"] is None else c["oct"][None]


@pytest.mark.parametrize("name", NAMES)
def test_transform_equals_the_reference(gpu, live, name):
    """every recorded case: 1, 2, 10, 17, 33, 128 and 255 children; NF 1, 16, 17; a frame of 1 200 slots on the (10, 4) and (3, 6)
    vocabularies with and without early leaves at levelsup 0, 2, 4, L + 3"""
    torch, ctx = gpu
    c = DC.cases()[name]
    got = device_transform(torch, ctx, dev_voc(ctx, c), c["desc"][None], octaves(c), c["levelsup"])
    for what, r in references(name, live):
        same(got, DC.as_outputs(c, r), "%s (%s)" % (name, what))


def test_batch_of_three_with_different_node_counts(gpu, live):
    torch, ctx = gpu
    names = [n for n in NAMES if n.startswith("batch3/")]
    cs = [DC.cases()[n] for n in names]
    assert len(cs) == 3 and len(set(id(c["voc"]) for c in cs)) == 1 and len(set(c["levelsup"] for c in cs)) == 1
    got = device_transform(torch, ctx, dev_voc(ctx, cs[0]), np.stack([c["desc"] for c in cs]), np.stack([c["oct"] for c in cs]), cs[0]["levelsup"])
    for which in range(2 if live is not None else 1):
        outs = [DC.as_outputs(c, references(n, live)[which][1]) for n, c in zip(names, cs)]
        ref = {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
        assert len(set(ref["nnode"].tolist())) == 3 and ref["nnode"][1] == 1 and ref["nnode"][2] == 0, ref["nnode"]
        same(got, ref, "B=3 (%d)" % which)


@pytest.mark.parametrize("name", ["case/interleaved_ids", "case/last_record_nearest", "synth/k10_L4_early/levelsup_0"])
def test_through_the_file(gpu, live, tmp_path, name):
    """gl_voc_load_file on the file the reference loads: the reference's word and node counts less the phantom, and the transform
    bits of gl_voc_create from arrays, which are the reference's"""
    from gmmloc_amd import bow
    torch, ctx = gpu
    c, r = DC.cases()[name], DC.recorded()[0][name]
    p = tmp_path / "voc.bin"
    synth.write_vocabulary_file(p, c["voc"])
    counts = [(r["voc_nodes"], r["voc_words"])]
    ref = oracle_lib.load_dbow2()
    if ref is not None:
        h = ref.load(p)
        i = ref.info(h)
        ref.destroy(h)
        counts.append((i["nodes"], i["words"]))
    dv = bow.Vocabulary.from_file(ctx, p)
    try:
        info, info_arrays = dv.info(), dev_voc(ctx, c).info()
        for nodes, words in counts:
            assert (info["nodes"], info["words"]) == (nodes - 1, words - 1)
        assert info == info_arrays
        got = device_transform(torch, ctx, dv, c["desc"][None], octaves(c), c["levelsup"])
    finally:
        dv.close()
    same(got, device_transform(torch, ctx, dev_voc(ctx, c), c["desc"][None], octaves(c), c["levelsup"]), name + " file / arrays")
    for what, rr in references(name, live):
        same(got, DC.as_outputs(c, rr), "%s from file (%s)" % (name, what))


def test_search_by_bow_on_device_made_and_reference_made_feature_vectors(gpu):
    """gl_search_by_bow on the synth_bow_pair whose feature vectors come once from the reference (recorded, uploaded) and once from
    gl_bow_transform on the same descriptors (never leaving the device): identical matches"""
    from gmmloc_amd import api, bow
    torch, ctx = gpu
    NN = 64
    sides = []
    for route in ("reference", "device"):
        pair = []
        for side, s in zip(("kf", "fr"), DC.bow_pair()):
            c = DC.cases()["bow_pair/dense/" + side]
            d = dict(angle=T(torch, s["angle"][None]), desc=T(torch, s["desc"][None]), has_mp=T(torch, s["has_mp"][None]))
            if route == "reference":
                r = DC.as_outputs(c, DC.recorded()[0]["bow_pair/dense/" + side], nn_cap=NN, fill=0)
                assert r["status"][0] == 0 and r["nnode"][0] > 4
                d.update({k: T(torch, r[k]) for k in bow.FV_KEYS})
            else:
                r = bow.transform(ctx, dev_voc(ctx, c), d["desc"], T(torch, c["oct"][None]), levelsup=c["levelsup"], nn_cap=NN, per_feature=False)
                d.update({k: r[k] for k in bow.FV_KEYS})
            pair.append(d)
        m, nm = api.search_by_bow(ctx, pair[0], pair[1])
        torch.cuda.synchronize()
        sides.append((m.cpu().numpy(), nm.cpu().numpy()))
    print("matches", sides[0][1])
    assert sides[0][1][0] > 0
    assert np.array_equal(sides[0][0], sides[1][0]) and np.array_equal(sides[0][1], sides[1][1])
