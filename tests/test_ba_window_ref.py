"""CPU: the two restatements of tests/ba_window_ref.py agree exactly on every scene of tests/ba_window_scenes.py, and the scenes meet
the conditions that keep tests/test_gpu_ba_window.py from passing vacuously - checked on the restatement alone."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import ba_window_ref as R
from tests import ba_window_scenes as S

WINDOW_KEYS = ("P", "F", "L", "nobs", "no_conn", "dropped") + R.WINDOW_ARRAYS


def same_window(a, b):
    return all(np.array_equal(a[k], b[k]) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype for k in WINDOW_KEYS)


@pytest.fixture(scope="module")
def geo(map_v1, gt_sync):
    return S.geometric_scene(map_v1[0], map_v1[1], gt_sync["V1_01_easy"])


@pytest.mark.parametrize("name", list(S.SCENES))
def test_the_two_restatements_agree(name):
    m, ba, rows = S.scene(name)
    for kf in rows[:(16 if name in S.SMALL else 2)]:
        a, b = R.connections_seq(m, int(kf)), R.connections_vec(m, int(kf))
        assert all(np.array_equal(a[k], b[k]) for k in a), (name, kf)
        assert same_window(R.window_seq(m, ba, int(kf)), R.window_vec(m, ba, int(kf))), (name, kf)


def test_the_two_restatements_agree_on_the_geometric_scene(geo):
    m, ba, kf = geo
    for k in range(m["kf_mp"].shape[0]):
        assert same_window(R.window_seq(m, ba, k), R.window_vec(m, ba, k)), k


def test_malformed_input_is_skipped_alike():
    m, ba, rows = S.scene("small")
    S.malform(m, ba, 5)
    for kf in rows:
        assert same_window(R.window_seq(m, ba, int(kf)), R.window_vec(m, ba, int(kf))), kf


def test_the_scenes_are_not_vacuous():
    kinds = {}
    for name in S.SMALL:
        m, ba, rows = S.scene(name)
        kinds[name] = S.window_kinds(m, ba, rows)
    assert kinds["tiny"]["single"].sum() >= 8 and not kinds["tiny"]["tie"].all()  # no observer reaches 15: the single-largest branch
    assert kinds["small"]["tie"].any() and not kinds["small"]["single"].any()  # a weight tie among the kept observers
    assert kinds["small"]["empty"].any() and kinds["tiny"]["empty"].any()  # an empty counter
    assert kinds["small"]["invalid_conn"].any()  # an invalid key-frame inside the covisible list
    assert kinds["small"]["invalid_observer"].any()  # ... and among a window point's observers
    assert kinds["small"]["shared_point"].any()  # a point held by two free key-frames
    assert kinds["small"]["mono"].any()
    assert kinds["clique"]["f0"].all() and kinds["clique"]["invalid_conn"].any()  # every key-frame free (or marked): no fixed pose
    assert kinds["small"]["f_pos"].any() and kinds["small"]["f0"].any()  # (f0 here: the isolated key-frame)
    # a point without an edge is dropped somewhere (the clique's invalid key-frame holds points nobody valid observes)
    m, ba, rows = S.scene("clique")
    assert any(R.window_seq(m, ba, int(kf))["dropped"] > 0 for kf in rows)


def test_the_geometric_window_is_inside_the_shapes_the_ba_tests_run(geo):
    """4 <= P <= 20, F >= 1, P + F <= 28, 300 <= L <= 1 500: the upper bounds are the largest shapes tests/test_gpu_ba.py runs in both
    bagen_modes"""
    m, ba, kf = geo
    w = R.window_seq(m, ba, kf)
    print("geometric window: P %d F %d L %d nobs %d dropped %d" % (w["P"], w["F"], w["L"], w["nobs"], w["dropped"]))
    assert 4 <= w["P"] <= 20 and w["F"] >= 1 and w["P"] + w["F"] <= 28 and 300 <= w["L"] <= 1500
    k = S.window_kinds(m, ba, [kf], [w])
    assert k["mono"][0] and k["invalid_conn"][0] and k["shared_point"][0] and w["prior"].sum() == 1
    assert (w["assoc"] >= 0).any() and (w["assoc"] < 0).any()


def test_the_oracle_optimises_the_geometric_window(geo, oracle, map_v1):
    m, ba, kf = geo
    w = R.window_seq(m, ba, kf)
    h = oracle.gmm_create(*map_v1)
    r = oracle.joint_optimization(h, api.Camera(), w["P"], w["F"], w["poses"], w["prior"], w["points"], w["assoc"], w["obs_ptr"], w["obs_pose"],
                                  w["obs_uvr"], w["obs_oct"])
    oracle.gmm_destroy(h)
    assert np.isfinite(r[0]).all() and np.isfinite(r[1]).all() and r[4] > 0
    assert not np.array_equal(r[0][:w["P"]], w["poses"][:w["P"]])


def test_a_point_without_an_edge_is_left_alone_by_the_oracle(geo, oracle, map_v1):
    """why gl_ba_window_build DROPS such a point: with it appended to the window (no observation, no association) the oracle returns
    it bit-identical, like g2o, whose active set never holds the vertex - so leaving it out of the window loses nothing"""
    m, ba, kf = geo
    w = R.window_seq(m, ba, kf)
    h = oracle.gmm_create(*map_v1)
    lone = np.array([[0.25, -0.5, 1.0]])
    r = oracle.joint_optimization(h, api.Camera(), w["P"], w["F"], w["poses"], w["prior"], np.concatenate([w["points"], lone]),
                                  np.concatenate([w["assoc"], [-1]]).astype(np.int32), np.concatenate([w["obs_ptr"], w["obs_ptr"][-1:]]), w["obs_pose"],
                                  w["obs_uvr"], w["obs_oct"])
    oracle.gmm_destroy(h)
    assert r[1][-1].tobytes() == lone[0].tobytes()
