"""The cases whose outputs the reference's own DBoW2 gave, as recorded in tests/golden/golden_dbow2_ref.npz (tools/record_dbow2_ref.py
writes it from oracle/_ref/libdbow2_ref.so): the inputs, regenerated here from the hand-built cases and from seeds, and the reader of the
recorded file.  tests/test_dbow2_ref.py holds the restatement, the declared expectations and the live library to it, tests/
test_gpu_dbow2_ref.py the device.

A case: voc, desc (NF,32) u8, oct (NF,) i32 or None (< 0: a padding slot - this project's notion; the reference is given the other slots,
compacted, and its feature indices are mapped back by `slots`), levelsup.  A recorded result, in the reference's compacted indices:
word i32, weight f32 (the bits), nid u32 (NID_UNSET: the reference left it unwritten), final i32 (the leaf's node id), fv = [(node id,
[feature indices])] in the reference's map order, overload (the vector overload was run and gave the same feature vector), voc_nodes /
voc_words (m_nodes.size() and size() of the loaded vocabulary)."""
import functools
import os

import numpy as np

from gmmloc_amd import synth
from tests import bow_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "golden_dbow2_ref.npz")
NID_UNSET = 0xFFFFFFFF
SYNTH = {"k10_L4": (10, 4, 21, 0.0), "k10_L4_early": (10, 4, 22, 0.15), "k3_L6": (3, 6, 23, 0.0), "k3_L6_early": (3, 6, 24, 0.15)}  # k, L, seed, early leaves
SYNTH_NF = 1200
DENSE = (4, 3, 12)  # the vocabulary of the searchByBoW pair: random descriptors, as test_gpu_bow's "dense"


@functools.lru_cache(maxsize=None)
def synth_voc(name):
    if name == "dense":
        v = synth.synth_vocabulary(*DENSE, flip_bits=1, dup_frac=0.0, stop_frac=0.05)
    else:
        k, L, seed, early = SYNTH[name]
        v = synth.synth_vocabulary(k, L, seed, early_leaf_frac=early)
    for a in v.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def synth_frame(name, NF, seed, pad_front=0, pad_back=0, pad_frac=0.0):
    """descriptors near the vocabulary's node descriptors; padding slots in front, behind and scattered"""
    desc = synth.synth_vocabulary_descriptors(synth_voc(name), NF, seed)
    rng = np.random.default_rng(seed + 5)
    octave = rng.integers(0, 8, NF).astype(np.int32)
    octave[:pad_front] = -1
    octave[NF - pad_back:] = -1 - rng.integers(0, 3, pad_back)
    octave[rng.uniform(size=NF) < pad_frac] = -1
    desc.setflags(write=False)
    octave.setflags(write=False)
    return desc, octave


def _batch3(name):
    """three frames of 40 slots with different node counts: a mixed frame, forty copies of one kept word's descriptor, padding only"""
    v = synth_voc(name)
    d0, o0 = synth_frame(name, 40, 7, 1, 2, 0.05)
    word = np.nonzero((np.asarray(v["is_leaf"]) != 0) & (v["weight"] > 0))[0][-1]  # a leaf of the last level that is no stopped word
    one = np.repeat(v["desc"][word][None], 40, axis=0)
    return [(d0, o0), (one, np.zeros(40, np.int32)), (d0, -np.ones(40, np.int32))]


@functools.lru_cache(maxsize=None)
def bow_pair():
    """the key-frame / frame pair of ORBmatcher::searchByBoW (synth.synth_bow_pair): two views of the same points -> (kf, fr)"""
    from gmmloc_amd import api
    return synth.synth_bow_pair(300, 280, 5, api.Camera())


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(voc, desc, oct, levelsup), in the order of the recorded file"""
    out = {}
    for name, c in BC.CASES.items():
        out["case/" + name] = dict(voc=c["voc"], desc=c["desc"], oct=c["oct"], levelsup=c["levelsup"])
    for name, (k, L, seed, early) in SYNTH.items():
        desc, octave = synth_frame(name, SYNTH_NF, 100 + seed, 5, 9, 0.03)
        for levelsup in (0, 2, 4, L + 3):
            out["synth/%s/levelsup_%d" % (name, levelsup)] = dict(voc=synth_voc(name), desc=desc, oct=octave, levelsup=levelsup)
    small = "k10_L4_early"
    for NF, pads in ((1, (0, 0, 0.0)), (16, (0, 0, 0.0)), (17, (2, 1, 0.0))):
        desc, octave = synth_frame(small, NF, 300 + NF, *pads)
        out["frame/%s/NF_%d" % (small, NF)] = dict(voc=synth_voc(small), desc=desc, oct=octave, levelsup=1)
    for b, (desc, octave) in enumerate(_batch3(small)):
        out["batch3/%s/%d" % (small, b)] = dict(voc=synth_voc(small), desc=desc, oct=octave, levelsup=1)
    for side, f in zip(("kf", "fr"), bow_pair()):
        out["bow_pair/dense/" + side] = dict(voc=synth_voc("dense"), desc=f["desc"], oct=f["oct"].astype(np.int32), levelsup=1)
    return out


def slots(c):
    """the slots of a case that are features, ascending: the reference's feature i is slot slots(c)[i]"""
    return np.arange(len(c["desc"])) if c["oct"] is None else np.nonzero(np.asarray(c["oct"]) >= 0)[0]


def dump_voc():
    """the small interleaved vocabulary whose node dump is recorded: early leaves, and the special weights in the first records"""
    v = {k: np.array(a) if isinstance(a, np.ndarray) else a for k, a in synth.synth_vocabulary(3, 3, 31, interleave=True, early_leaf_frac=0.2).items()}
    v["weight"][:3] = [np.float32("nan"), np.float32(-0.0), BC.F32_DENORM_MIN]
    return v


DUMP_KEYS = ("info", "parent", "desc", "weight", "word_id", "child_ptr", "child_ids")


def live(ref, tmp_dir):
    """every case and the node dump through the live library `ref` (tests.oracle_lib.DBoW2Ref): each vocabulary written to a file under
    tmp_dir by synth.write_vocabulary_file and read by the reference's loadFromBinaryFile -> ({name: result}, dump, {name: the
    vector overload's own feature vector or None})"""
    loaded, results, overload_fv = {}, {}, {}
    try:
        for name, c in cases().items():
            if id(c["voc"]) not in loaded:
                p = os.path.join(str(tmp_dir), "voc_%d.bin" % len(loaded))
                synth.write_vocabulary_file(p, c["voc"])
                loaded[id(c["voc"])] = ref.load(p)
            h = loaded[id(c["voc"])]
            d = np.ascontiguousarray(c["desc"][slots(c)])
            word, weight, nid, final = ref.transform(h, d, c["levelsup"])
            fa, fb, unwritten = ref.frame(h, d, c["levelsup"])
            assert unwritten == int((nid == NID_UNSET).sum()) and (fb is None) == (unwritten > 0)
            i = ref.info(h)
            results[name] = dict(word=word, weight=weight, nid=nid, final=final, fv=fa, overload=fb is not None, levelsup=c["levelsup"],
                                 voc_nodes=i["nodes"], voc_words=i["words"])
            overload_fv[name] = fb
        p = os.path.join(str(tmp_dir), "voc_dump.bin")
        synth.write_vocabulary_file(p, dump_voc())
        h = ref.load(p)
        loaded["dump"] = h
        dump = ref.nodes(h)
        i = ref.info(h)
        dump["info"] = np.array([i["nodes"], i["words"], i["k"], i["L"]], np.int32)
    finally:
        for h in loaded.values():
            ref.destroy(h)
    return results, dump, overload_fv


def pack(results, dump):
    """{name: result} in the order of cases(), the node dump -> the arrays of the file (data only)"""
    names = list(results)
    assert names == list(cases())
    cat = lambda key, dt: np.concatenate([np.asarray(results[n][key], dt).reshape(-1) for n in names]) if names else np.zeros(0, dt)
    out = dict(names=np.array(names), levelsup=np.array([cases()[n]["levelsup"] for n in names], np.int32),
               n_feat=np.array([len(results[n]["word"]) for n in names], np.int32), word=cat("word", np.int32),
               weight_bits=np.concatenate([np.asarray(results[n]["weight"], np.float32).view(np.uint32) for n in names]),
               nid=cat("nid", np.uint32), final=cat("final", np.int32), overload=np.array([results[n]["overload"] for n in names], np.uint8),
               n_node=np.array([len(results[n]["fv"]) for n in names], np.int32),
               voc_nodes=np.array([results[n]["voc_nodes"] for n in names], np.int32), voc_words=np.array([results[n]["voc_words"] for n in names], np.int32))
    out["node_id"] = np.array([nid for n in names for nid, _ in results[n]["fv"]], np.int32)
    out["node_cnt"] = np.array([len(f) for n in names for _, f in results[n]["fv"]], np.int32)
    out["node_idx"] = np.array([i for n in names for _, f in results[n]["fv"] for i in f], np.int32)
    for k in DUMP_KEYS:
        out["dump_" + k] = np.asarray(dump[k]).view(np.uint32) if k == "weight" else np.asarray(dump[k])
    return out


@functools.lru_cache(maxsize=None)
def recorded():
    """the file -> ({name: result}, node dump); read-only arrays"""
    d = np.load(PATH)
    res = {}
    fa = na = ia = 0
    for i, name in enumerate(d["names"].tolist()):
        nf, nn = int(d["n_feat"][i]), int(d["n_node"][i])
        cnt = d["node_cnt"][na:na + nn]
        fv = []
        for r in range(nn):
            fv.append((int(d["node_id"][na + r]), d["node_idx"][ia:ia + int(cnt[r])].tolist()))
            ia += int(cnt[r])
        res[name] = dict(word=d["word"][fa:fa + nf], weight=d["weight_bits"][fa:fa + nf].view(np.float32), nid=d["nid"][fa:fa + nf],
                         final=d["final"][fa:fa + nf], fv=fv, overload=bool(d["overload"][i]), levelsup=int(d["levelsup"][i]),
                         voc_nodes=int(d["voc_nodes"][i]), voc_words=int(d["voc_words"][i]))
        fa, na = fa + nf, na + nn
    assert (fa, na, ia) == (len(d["word"]), len(d["node_id"]), len(d["node_idx"]))
    dump = {k: (d["dump_" + k].view(np.float32) if k == "weight" else d["dump_" + k]) for k in DUMP_KEYS}
    return res, dump


def node(r):
    """the node of every feature as the reference gives it: nid, and the final node it reports itself where it left nid unwritten"""
    return np.where(r["nid"] == NID_UNSET, r["final"].astype(np.int64), r["nid"].astype(np.int64)).astype(np.int32)


def as_outputs(c, r, nn_cap=None, fill=-7):
    """a recorded result as the arrays of a one-frame gl_bow_transform on buffers filled with `fill` (compacted feature indices mapped
    back to slots; a padding slot: -1 / -1 / 0.0f) -> dict of (1, ...) arrays with the keys of tests.test_gpu_bow_cases.OUT_KEYS"""
    from tests import bow_ref as R
    NF, s = len(c["desc"]), slots(c)
    word, nd, weight = -np.ones(NF, np.int32), -np.ones(NF, np.int32), np.zeros(NF, np.float32)
    word[s], nd[s], weight[s] = r["word"], node(r), r["weight"]
    fv = [(n, [int(s[i]) for i in f]) for n, f in r["fv"]]
    nnode, node_id, node_ptr, node_idx, status = R.csr(fv, NF, NF if nn_cap is None else nn_cap, fill)
    return dict(word_id=word[None], node=nd[None], weight=weight[None], nnode=np.array([nnode], np.int32), node_id=node_id[None],
                node_ptr=node_ptr[None], node_idx=node_idx[None], status=np.array([status], np.int32))
