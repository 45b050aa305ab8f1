"""gl_voc_create / gl_bow_transform on the device against the declared outputs of tests/bow_cases.py: word, node and weight bits per
feature, and the feature vector as CSR on sentinel-filled buffers (what lies behind a frame's counts keeps the sentinel)."""
import functools

import numpy as np
import pytest

from tests import bow_cases as BC
from tests import bow_ref as R
from tests import gpu_helpers
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (the fixture is autouse)

pytestmark = pytest.mark.gpu
FILL = -7
OUT_KEYS = ("word_id", "node", "weight", "nnode", "node_id", "node_ptr", "node_idx", "status")


T = functools.partial(gpu_helpers.T, copy=True)  # (a copy: the shared inputs are read-only arrays)


def device_voc(ctx, v):
    from gmmloc_amd import bow
    return bow.Vocabulary.from_arrays(ctx, v["parent"], v["desc"], v["weight"], v["is_leaf"], v["k"], v["L"])


def device_transform(torch, ctx, dv, desc, octave=None, levelsup=4, nn_cap=None, fill=FILL):
    """gl_bow_transform for desc (B,NF,32) on outputs filled with `fill` -> dict of host arrays (OUT_KEYS)"""
    from gmmloc_amd import bow
    B, NF = desc.shape[:2]
    nn_cap = NF if nn_cap is None else nn_cap
    out = bow.feature_vector_alloc(B, NF, nn_cap, fill=fill)
    out.update(word_id=torch.full((B, NF), fill, dtype=torch.int32, device="cuda"), node=torch.full((B, NF), fill, dtype=torch.int32, device="cuda"),
               weight=torch.full((B, NF), float(fill), dtype=torch.float32, device="cuda"), status=torch.full((B,), fill, dtype=torch.int32, device="cuda"))
    d = T(torch, desc)
    before = d.clone()
    r = bow.transform(ctx, dv, d, None if octave is None else T(torch, octave), levelsup=levelsup, out=out)
    torch.cuda.synchronize()
    assert torch.equal(d, before), "the descriptors were written"
    return {k: r[k].cpu().numpy() for k in OUT_KEYS}


def same(got, ref, what=""):
    """every output array, bit for bit (the weights as bit patterns: NaN and -0.0f included)"""
    for k in OUT_KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero(a.view(np.int32).reshape(-1) != b.view(np.int32).reshape(-1))[0]
            raise AssertionError("%s %s: %d entries differ, first at %d: %r != %r" % (what, k, len(bad), bad[0], a.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]]))


def declared(c, nn_cap=None):
    """a case's declared outputs as the arrays of a one-frame call"""
    e = c["expect"]
    NF = len(c["desc"])
    nnode, node_id, node_ptr, node_idx, status = R.csr(e["fv"], NF, NF if nn_cap is None else nn_cap, FILL)
    return dict(word_id=e["word_id"][None], node=e["node"][None], weight=e["weight"][None], nnode=np.array([nnode], np.int32), node_id=node_id[None],
                node_ptr=node_ptr[None], node_idx=node_idx[None], status=np.array([status], np.int32))


@pytest.mark.parametrize("name", list(BC.CASES))
def test_case(gpu, name):
    torch, ctx = gpu
    c = BC.CASES[name]
    dv = device_voc(ctx, c["voc"])
    try:
        got = device_transform(torch, ctx, dv, c["desc"][None], None if c["oct"] is None else c["oct"][None], c["levelsup"])
    finally:
        dv.close()
    same(got, declared(c), name)


def test_info(gpu):
    torch, ctx = gpu
    for name, want in (("children_255", dict(nodes=256, words=255, k=255, L=1, max_children=255, min_leaf_level=1)),
                       ("shallow_leaf", dict(nodes=9, words=5, k=2, L=3, max_children=2, min_leaf_level=1)),
                       ("levelsup_0", dict(nodes=15, words=8, k=2, L=3, max_children=2, min_leaf_level=3))):
        dv = device_voc(ctx, BC.CASES[name]["voc"])
        info = dv.info()
        dv.close()
        assert info.pop("device_bytes") == 48 * (want["nodes"] - 1)
        assert info == want, name


def test_vocabulary_from_file_equals_from_arrays(gpu, tmp_path):
    from gmmloc_amd import bow, synth
    torch, ctx = gpu
    c = BC.CASES["interleaved_ids"]
    p = tmp_path / "voc.bin"
    synth.write_vocabulary_file(p, c["voc"])
    dv = bow.Vocabulary.from_file(ctx, p)
    try:
        assert dv.info()["nodes"] == 7
        same(device_transform(torch, ctx, dv, c["desc"][None], None, 0), declared(c), "from_file")
    finally:
        dv.close()


def test_inconsistent_arrays_are_argument_errors(gpu):
    from gmmloc_amd import api, bow
    torch, ctx = gpu
    v = BC.CASES["interleaved_ids"]["voc"]
    for key, at, val in (("parent", 2, 3), ("parent", 2, -1), ("parent", 5, 3), ("is_leaf", 0, 1), ("is_leaf", 5, 0)):
        w = {k: np.array(a) for k, a in v.items()}
        w[key][at] = val
        with pytest.raises(api.GLError, match="error -1"):
            bow.Vocabulary.from_arrays(ctx, w["parent"], w["desc"], w["weight"], w["is_leaf"], 2, 2)


def test_argument_errors_leave_the_outputs_untouched(gpu):
    from gmmloc_amd import api, bow
    torch, ctx = gpu
    c = BC.CASES["interleaved_ids"]
    dv = device_voc(ctx, c["voc"])
    try:
        d = T(torch, c["desc"][None])
        for kw in (dict(levelsup=-1), dict(nn_cap=0), dict(nn_cap=4097)):
            out = bow.feature_vector_alloc(1, 5, kw.get("nn_cap", 5), fill=FILL)  # (transform takes NNcap from node_id)
            out["status"] = torch.full((1,), FILL, dtype=torch.int32, device="cuda")
            with pytest.raises(api.GLError, match="error -1"):
                bow.transform(ctx, dv, d, None, out=dict(out), levelsup=kw.get("levelsup", 4))
            torch.cuda.synchronize()
            assert all(bool((t == FILL).all()) for t in out.values()), kw
        big = torch.zeros((1, 4097, 32), dtype=torch.uint8, device="cuda")
        with pytest.raises(api.GLError, match="error -1"):
            bow.transform(ctx, dv, big, None)
    finally:
        dv.close()
