"""gl_bow_transform on the device against the sequential restatement (tests/bow_ref.py), bit for bit: frame shapes and padding, batches,
the capacity rule, randomised vocabularies up to the shape of the ORB vocabulary, the consumers of the feature vector downstream, the
context's history, and the C++ adapter.  The hand-built cases are in tests/test_gpu_bow_cases.py."""
import functools
import os

import numpy as np
import pytest

from gmmloc_amd import synth
from tests import bow_ref as R
from tests import cpp_driver
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (autouse fixture)
from tests.test_gpu_bow_cases import FILL, OUT_KEYS, T, device_transform, device_voc, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- vocabularies: made once, with their restatement trees and device objects -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_voc(name):
    """small: 4 children, depth 3, some early leaves (84 records at most; level 2 holds at most 16 nodes, so the 1 200 or 4 096 features
    of a frame crowd into a few nodes, each spread over many waves).  dense: random descriptors (for dense ORB-like features).
    k10_L4 / k10_L6: the randomised vocabularies of the issue; the second has the shape of the ORB vocabulary (1 111 110 records)."""
    v = {"small": lambda: synth.synth_vocabulary(4, 3, 11, early_leaf_frac=0.15, stop_frac=0.15),
         "dense": lambda: synth.synth_vocabulary(4, 3, 12, flip_bits=1, dup_frac=0.0, stop_frac=0.05),
         "k10_L4": lambda: synth.synth_vocabulary(10, 4, 13),
         "k10_L6": lambda: synth.synth_vocabulary(10, 6, 14)}[name]()
    return v, R.Tree(v)


_dev = {}


def dev_voc(ctx, name):
    if name not in _dev:
        _dev[name] = device_voc(ctx, host_voc(name)[0])
    return _dev[name]


@functools.lru_cache(maxsize=None)
def frame(name, NF, seed, pad_front=0, pad_back=0, pad_frac=0.0):
    """descriptors near the vocabulary's node descriptors, octaves with padding slots (< 0) in front, behind and scattered"""
    v, _ = host_voc(name)
    desc = synth.synth_vocabulary_descriptors(v, NF, seed)
    rng = np.random.default_rng(seed + 5)
    octave = rng.integers(0, 8, NF).astype(np.int32)
    octave[:pad_front] = -1
    octave[NF - pad_back:] = -1 - rng.integers(0, 3, pad_back)
    octave[rng.uniform(size=NF) < pad_frac] = -1
    desc.setflags(write=False)
    octave.setflags(write=False)
    return desc, octave


@functools.lru_cache(maxsize=None)
def restated(name, NF, seed, pads, levelsup, nn_cap=None):
    """the restatement of one frame, computed once (read-only arrays)"""
    desc, octave = frame(name, NF, seed, *pads)
    out = R.transform_batch(host_voc(name)[1], desc[None], octave[None], levelsup, nn_cap, FILL)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- frame shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NF,pads", [(1, (0, 0, 0.0)), (3, (1, 1, 0.0)), (16, (0, 0, 0.0)), (17, (2, 1, 0.0)), (1200, (5, 9, 0.03)), (4096, (3, 70, 0.02))])
def test_frame_shapes(gpu, NF, pads):
    """NF at, below and above a row of 16 and a workgroup's 16 features, the chain's 1 200, the limit 4 096 (a sort of 4 096 keys);
    padding slots at both ends; levelsup 1: a few crowded nodes whose features come from every wave of the frame"""
    torch, ctx = gpu
    desc, octave = frame("small", NF, 100 + NF, *pads)
    ref = restated("small", NF, 100 + NF, pads, 1)
    got = device_transform(torch, ctx, dev_voc(ctx, "small"), desc[None], octave[None], 1)
    same(got, ref, "NF=%d" % NF)
    if NF >= 1200:
        n = int(ref["nnode"][0])
        sizes = np.diff(ref["node_ptr"][0, :n + 1])
        print("NF", NF, "nodes", n, "largest node", sizes.max(), "kept", int(ref["node_ptr"][0, n]))
        assert sizes.max() > 64  # one node's features span several waves: index order inside the node is the sort's work


def test_no_octaves_means_every_slot_is_a_feature(gpu):
    torch, ctx = gpu
    desc, _ = frame("small", 17, 117, 2, 1, 0.0)
    ref = R.transform_batch(host_voc("small")[1], desc[None], None, 1, None, FILL)
    same(device_transform(torch, ctx, dev_voc(ctx, "small"), desc[None], None, 1), ref, "oct = NULL")


def _batch3():
    """three frames of 40 slots with different node counts: all of level 2, one node's worth, nothing (every slot padding)"""
    v, tree = host_voc("small")
    d0, o0 = frame("small", 40, 7, 1, 2, 0.05)
    lvl2 = [i + 1 for i in np.nonzero(np.asarray(v["is_leaf"]) == 0)[0] if v["parent"][i] != 0]  # the inner nodes of level 2
    word = np.nonzero(np.isin(v["parent"], lvl2) & (v["weight"] > 0))[0][0]  # a leaf of level 3 that is no stopped word
    one = np.repeat(v["desc"][word][None], 40, axis=0)  # forty copies of it: one node
    desc = np.stack([d0, one, d0])
    octave = np.stack([o0, np.zeros(40, np.int32), -np.ones(40, np.int32)])
    return desc, octave, tree


def test_batch_of_three_with_different_node_counts(gpu):
    torch, ctx = gpu
    desc, octave, tree = _batch3()
    ref = R.transform_batch(tree, desc, octave, 1, None, FILL)
    assert len(set(ref["nnode"].tolist())) == 3 and ref["nnode"][2] == 0, ref["nnode"]
    same(device_transform(torch, ctx, dev_voc(ctx, "small"), desc, octave, 1), ref, "B=3")


# ---- capacity ----------------------------------------------------------------------------------------------------------------------------
def test_capacity_exact_and_one_below(gpu):
    """NNcap = the largest frame's node count: nothing truncated.  One below: that frame alone gets the bit and its true count, its CSR
    arrays keep the sentinel, its per-feature outputs are complete; the other frames of the batch are unchanged to the byte."""
    torch, ctx = gpu
    desc, octave, tree = _batch3()
    full = R.transform_batch(tree, desc, octave, 1, None, FILL)
    n = int(full["nnode"].max())
    assert n >= 3 and (full["nnode"] == n).sum() == 1
    for cap, trunc in ((n, False), (n - 1, True)):
        ref = R.transform_batch(tree, desc, octave, 1, cap, FILL)
        assert ref["status"].tolist() == [int(trunc), 0, 0] and ref["nnode"].tolist() == full["nnode"].tolist()
        if trunc:
            assert all((ref[k][0] == FILL).all() for k in ("node_id", "node_ptr", "node_idx")) and (ref["word_id"][0] == full["word_id"][0]).all()
        same(device_transform(torch, ctx, dev_voc(ctx, "small"), desc, octave, 1, nn_cap=cap), ref, "NNcap=%d" % cap)


# ---- levels on a random vocabulary with early leaves -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("levelsup", [0, 2, 3, 6])
def test_levels(gpu, levelsup):
    """levelsup 0, L - 1, L, L + 3 on the vocabulary with leaves at levels 1 .. 3 (shallow leaves at every level asked for)"""
    torch, ctx = gpu
    desc, octave = frame("small", 200, 31, 0, 0, 0.0)
    ref = restated("small", 200, 31, (0, 0, 0.0), levelsup)
    same(device_transform(torch, ctx, dev_voc(ctx, "small"), desc[None], octave[None], levelsup), ref, "levelsup=%d" % levelsup)


# ---- randomised vocabularies ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", ["k10_L4", "k10_L6"])
def test_randomised_vocabulary(gpu, name, seed):
    torch, ctx = gpu
    desc, octave = frame(name, 1200, seed, 0, 0, 0.01)
    ref = restated(name, 1200, seed, (0, 0, 0.01), 4)
    got = device_transform(torch, ctx, dev_voc(ctx, name), desc[None], octave[None], 4)
    same(got, ref, "%s seed %d" % (name, seed))
    if name == "k10_L6":
        info = dev_voc(ctx, name).info()
        assert (info["nodes"], info["words"], info["max_children"], info["min_leaf_level"]) == (1111111, 1000000, 10, 6)


# ---- downstream: the consumers read what the transform wrote ------------------------------------------------------------------------------------
def _fv_keys(r, b=0):
    n = int(r["nnode"][b])
    return dict(node_id=r["node_id"][b, :n].copy(), node_ptr=r["node_ptr"][b, :n + 1].copy(), node_idx=r["node_idx"][b, :int(r["node_ptr"][b, n])].copy())


def test_search_by_bow_on_device_made_feature_vectors(gpu):
    """gl_search_by_bow on a synth_bow_pair whose feature vectors come once from the restatement (uploaded) and once from
    gl_bow_transform on the same descriptors (never leaving the device): identical matches"""
    from gmmloc_amd import api, bow
    torch, ctx = gpu
    cam = api.Camera()
    kf, fr = synth.synth_bow_pair(300, 280, 5, cam)
    tree, dv = host_voc("dense")[1], dev_voc(ctx, "dense")
    NN = 64
    sides = []
    for route in ("restated", "device"):
        pair = []
        for s in (kf, fr):
            N = len(s["oct"])
            d = dict(angle=T(torch, s["angle"][None]), desc=T(torch, s["desc"][None]), has_mp=T(torch, s["has_mp"][None]))
            if route == "restated":
                r = R.transform_batch(tree, s["desc"][None], s["oct"][None], 1, NN, 0)
                assert r["status"][0] == 0 and r["nnode"][0] > 4
                d.update({k: T(torch, r[k]) for k in bow.FV_KEYS})
            else:
                r = bow.transform(ctx, dv, d["desc"], T(torch, s["oct"][None].astype(np.int32)), levelsup=1, nn_cap=NN, per_feature=False)
                d.update({k: r[k] for k in bow.FV_KEYS})
            pair.append(d)
        m, nm = api.search_by_bow(ctx, pair[0], pair[1])
        torch.cuda.synchronize()
        sides.append((m.cpu().numpy(), nm.cpu().numpy()))
    print("matches", sides[0][1])
    assert sides[0][1][0] > 0
    assert np.array_equal(sides[0][0], sides[1][0]) and np.array_equal(sides[0][1], sides[1][1])


def test_create_map_points_on_rows_written_by_transform_into_tables(gpu):
    """one key-frame through gl_create_map_points_from_map with the feature-vector rows of every key-frame once uploaded from the
    restatement and once written in place by transform_into_tables: every output array equal"""
    from gmmloc_amd import api, bow, map_grow
    from tests import create_points_cases as cc
    from tests.test_gpu_create_points import dev_points, dev_scene
    torch, ctx = gpu
    sc = cc.generated(65, 6, 41)
    n_kf, NFK, NN = sc.kt["desc"].shape[0], sc.NFK, 24
    tree, dv = host_voc("dense")[1], dev_voc(ctx, "dense")
    r = R.transform_batch(tree, sc.kt["desc"], sc.ba["kf_oct"], 1, NN, 0)
    assert (r["status"] == 0).all()
    md, bd, kt = dev_scene(torch, sc)
    up = dict(kt, **{k: T(torch, r[k]) for k in bow.FV_KEYS})
    made = dict(kt, **bow.feature_vector_alloc(n_kf, NFK, NN))
    for row in range(n_kf):
        st = bow.transform_into_tables(ctx, dv, made, row, oct=bd["kf_oct"][row], levelsup=1)
        assert int(st[0]) == 0
    torch.cuda.synchronize()
    for k in bow.FV_KEYS:
        assert np.array_equal(made[k].cpu().numpy(), r[k]), k
    conn, mb = np.arange(1, 5, dtype=np.int32), map_grow.default_mb(api.Camera(**sc.cam))
    a = dev_points(torch, ctx, sc, conn, 4, 0, 4, mb, sc.NMP, dev=(md, bd, up))
    b = dev_points(torch, ctx, sc, conn, 4, 0, 4, mb, sc.NMP, dev=(md, bd, made))
    print("matches per neighbour", a["nb_stats"][:, 2].tolist(), "new points", a["n_new"])
    assert a["nb_stats"][:, 2].sum() > 0
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


# ---- context history -----------------------------------------------------------------------------------------------------------------------
def _small_call(torch, ctx):
    desc, octave = frame("small", 17, 117, 2, 1, 0.0)
    dv = device_voc(ctx, host_voc("small")[0])
    try:
        return device_transform(torch, ctx, dv, desc[None], octave[None], 1)
    finally:
        dv.close()


def _large_call(torch, ctx):
    desc, octave = frame("small", 4096, 100 + 4096, 3, 70, 0.02)
    dv = device_voc(ctx, host_voc("small")[0])
    try:
        return device_transform(torch, ctx, dv, np.stack([desc] * 3), np.stack([octave] * 3), 0)
    finally:
        dv.close()


def test_same_bits_whatever_the_context_has_been_through(gpu):
    """the first call of a new context == after larger calls == on scratch filled with 0x00 / 0xFF, as it stands and as it is allocated"""
    from tests.context_cases import close_context, new_context
    from tests.context_pass import on_new_context, run
    torch = gpu[0]
    ref = restated("small", 17, 117, (2, 1, 0.0), 1)
    same(on_new_context(torch, _small_call), ref, "new context")
    ctx = new_context()
    try:
        run(_large_call, torch, ctx)
        same(run(_small_call, torch, ctx), ref, "after a larger call")
        for v in (0x00, 0xFF):
            ctx.set_option("test_scratch_fill", v)
            same(run(_small_call, torch, ctx), ref, "blocks filled with 0x%02X" % v)
    finally:
        close_context(ctx)
    for v in (0x00, 0xFF):
        same(on_new_context(torch, _small_call, fill=v), ref, "new context, blocks filled with 0x%02X as they are allocated" % v)


# ---- the C++ adapter ---------------------------------------------------------------------------------------------------------------------------
def test_cpp_adapter_gives_the_bytes_of_the_python_host(gpu, tmp_path):
    from gmmloc_amd import bow
    torch, ctx = gpu
    exe = cpp_driver.build("bow_check", tmp_path)
    v = host_voc("small")[0]
    synth.write_vocabulary_file(tmp_path / "voc.bin", v)
    N, NN, levelsup = 203, 16, 1
    desc, octave = frame("small", N, 77, 3, 2, 0.04)
    with open(tmp_path / "frame.bin", "wb") as fh:
        np.array([N, levelsup, NN], np.int32).tofile(fh)
        desc.tofile(fh)
        octave.tofile(fh)
    r = cpp_driver.run(exe, os.path.join(GOLDEN, "v1.gmm"), tmp_path / "voc.bin", tmp_path / "frame.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    out = open(tmp_path / "out.bin", "rb")
    rd = lambda n: np.fromfile(out, np.int32, n)
    # bowTransform: every slot a feature, NNcap = N
    dv = dev_voc(ctx, "small")
    py = {k: t.cpu().numpy() for k, t in bow.transform(ctx, dv, T(torch, desc[None]), None, levelsup=levelsup, per_feature=False).items()}
    want = _fv_keys(py)
    nnode, nidx = rd(2)
    assert (nnode, nidx) == (len(want["node_id"]), len(want["node_idx"])) and nnode > 3
    for k, n in (("node_id", nnode), ("node_ptr", nnode + 1), ("node_idx", nidx)):
        assert rd(n).tobytes() == want[k].tobytes(), k
    # bowTransformIntoTables: row 1 of two, the resident octaves as padding, the rest of the tables untouched
    F9 = np.frombuffer(b"\xf9" * 4, np.int32)[0]
    tables = dict(desc=T(torch, np.stack([np.zeros_like(desc), desc])), **bow.feature_vector_alloc(2, N, NN, fill=int(F9)))
    st = bow.transform_into_tables(ctx, dv, tables, 1, oct=T(torch, octave), levelsup=levelsup)
    torch.cuda.synchronize()
    assert rd(1)[0] == int(st[0]) == 0
    for k in bow.FV_KEYS:
        h = tables[k].cpu().numpy()
        assert rd(h.size).tobytes() == h.tobytes(), k
        assert (h[0] == F9).all(), k
    assert out.read() == b""
