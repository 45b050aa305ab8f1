"""CPU: the sequential model of the two depth-ordered walks (tests/key_frame_create_ref.py) gives every output the hand-built cases of
tests/key_frame_create_cases.py declare - with the C++ oracle's checkMapAssociation and with oracle/numpy_ref.py's - the pairs differ
where they say, and the library and its binding table hold the two entry points."""
import numpy as np
import pytest

from oracle import numpy_ref
from tests import key_frame_create_cases as cc
from tests import key_frame_create_ref as ref
from tests import keyframe_cases as kc

INT_KEYS = ("new_feat", "new_assoc", "new_ref_kf", "att_mp", "att_kf", "att_feat", "n_new", "feat_new", "stats")


def depth_points(c):
    """the pts0 a case implies: (0, 0, depth) for every entry - the camera looks along z from the origin - zeros elsewhere"""
    p = np.zeros((c.NF, 3))
    for i, f in enumerate(c.feats):
        if f["depth"] > 0 and 0 <= f["oct"] <= 7:
            # (+inf: x = y = inf 0 = NaN in the camera frame, and the rotation's cross products carry them into z: three NaN)
            p[i] = [0.0, 0.0, f["depth"]] if np.isfinite(f["depth"]) else [np.nan] * 3
    return p


def check_stereo(c, o):
    """o: the outputs of one key-frame with the lists cut to n_new, against everything the case declares"""
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(o[k]), np.asarray(c.want[k])), (c.name, k, o[k], c.want[k])
    assert np.allclose(o["pts0"], depth_points(c), rtol=0, atol=1e-9, equal_nan=True), (c.name, "pts0")
    for r, i in enumerate(c.want["new_feat"]):
        same = np.array_equal(o["new_pos"][r], o["pts0"][i], equal_nan=True)
        assert same != (i in c.want["moved"]), (c.name, "new_pos", r, i)


def check_temporal(c, o, before):
    for k in ("temp_flag", "n_temp", "stats", "last_valid"):
        assert np.array_equal(np.asarray(o[k]), np.asarray(c.want[k])), (c.name, k, o[k], c.want[k])
    p0 = depth_points(c)
    for i in range(c.NF):
        if i in c.want["created"]:
            assert np.allclose(o["last_pt"][i], p0[i], rtol=0, atol=1e-9, equal_nan=True) and o["last_observed"][i] == 0, (c.name, i)
            assert np.array_equal(o["last_desc"][i], c.fr["feat_desc"][i]), (c.name, i)
        else:
            for k in before:
                assert np.array_equal(o[k][i], before[k][i]), (c.name, "row %d of %s changed" % (i, k))


def model(c, backend):
    if c.call == "temporal":
        return ref.temporal_walk(c.cam, c.fr, cc.last_rows(c.NF), c.th)
    with kc.Ref(backend, c.mean, c.cov) as r:
        return ref.stereo_walk(c.cam, c.fr, ref.check_with(r, c.cam, c.fr), cc.MP_BASE, c.check_depth, c.th, cc.KF_ROW)


@pytest.mark.parametrize("backend", ["oracle", "numpy_ref"])
@pytest.mark.parametrize("name", cc.STEREO)
def test_stereo_case_declared_outputs(oracle, name, backend):
    c = cc.CASES[name]
    check_stereo(c, model(c, oracle if backend == "oracle" else numpy_ref))


@pytest.mark.parametrize("name", cc.TEMPORAL)
def test_temporal_case_declared_outputs(name):
    c = cc.CASES[name]
    check_temporal(c, model(c, None), cc.last_rows(c.NF))


def test_pairs_differ_where_declared():
    for a, b, elems in cc.PAIRS:
        sa, sb = cc.CASES[a].want["stats"], cc.CASES[b].want["stats"]
        assert tuple(np.nonzero(sa != sb)[0]) == tuple(sorted(elems)), (a, b, sa, sb)


def test_every_decision_has_a_case_on_each_side():
    seen = {}
    for c in cc.CASES.values():
        seen.setdefault(c.decision, set()).add(c.side)
    assert set(seen) == set(cc.DECISIONS) and all(len(v) >= 2 for v in seen.values()), seen


def test_table_check_equals_the_live_check():
    """the model run on per-feature results recorded beforehand (how the device's walk is isolated) = the model with the check inside"""
    c = cc.CASES["check_mixed_frame"]
    with kc.Ref(numpy_ref, c.mean, c.cov) as r:
        live = ref.check_with(r, c.cam, c.fr)
        p0 = depth_points(c)
        rec = [live(i, p0[i]) if c.fr["ncand"][i] > 0 else (-1, p0[i]) for i in range(c.NF)]
        a = ref.stereo_walk(c.cam, c.fr, live, cc.MP_BASE, 1, c.th, cc.KF_ROW)
    b = ref.stereo_walk(c.cam, c.fr, ref.check_table([x[0] for x in rec], [x[1] for x in rec]), cc.MP_BASE, 1, c.th, cc.KF_ROW)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_library_and_binding_table_hold_both_entry_points():
    from gmmloc_amd import _lib, api
    lib = _lib.load()
    for n in ("gl_create_stereo_points", "gl_create_temporal_points"):
        assert n in lib._gl_signatures and n not in lib._gl_missing and hasattr(lib, n), n
    assert callable(api.create_stereo_points) and callable(api.create_temporal_points)
