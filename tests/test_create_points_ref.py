"""CPU: the sequential model of createMapPoints on the resident map (tests/create_points_ref.py) gives the outputs every hand-built case
of tests/create_points_cases.py declares - with the C++ oracle's searchForTriangulation / createMapPoints and with numpy_ref's - and the
numpy statement of the device's fundamental matrix / epipole agrees with synth.fundamental_and_epipole inside the forward-error bound of
the product chain."""
import numpy as np
import pytest

from gmmloc_amd import api, synth
from oracle import numpy_ref
from tests import create_points_cases as cc
from tests import create_points_ref as ref
from tests import keyframe_cases as kc

f32, f64 = np.float32, np.float64
INT_KEYS = ref.LIST_KEYS + ref.ATT_KEYS + ("n_new", "n_attach", "feat_new", "nb_stats", "skip", "status")


def functions(backend, r, cam, scale_factor=1.2):
    """(search, create) of the model on one of the two CPU implementations; r: keyframe_cases.Ref of the case's GMM on it"""
    def search(kf1, kf2, fmat, epipole):
        return backend.search_for_triangulation(kf1, kf2, fmat, epipole, only_stereo=False, check_orientation=False, scale_factor=scale_factor)[0]

    def create(**a):
        return r.cmp(cam, *[a[k] for k in kc.CMP_KEYS], scale_factor)
    return search, create


def run_model(c, backend, **kw):
    with kc.Ref(backend, cc.MEAN, cc.COV) as r:
        search, create = functions(backend, r, cc.CAM)
        return ref.create_points(cc.CAM, c.map, c.ba, c.kt, c.kf_row, c.conn_kf, c.n_conn, c.first_nb, c.nn, c.mb, cc.MP_BASE, search, create, **kw)


def check_ints(o, want, what):
    for k in INT_KEYS:
        a, b = np.asarray(o[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a == b).all(), (what, k, a, b)


@pytest.mark.parametrize("name", sorted(cc.CASES))
@pytest.mark.parametrize("backend", ["oracle", "numpy_ref"])
def test_model_gives_the_declared_outputs(name, backend, request):
    c = cc.CASES[name]
    b = numpy_ref if backend == "numpy_ref" else request.getfixturevalue("oracle")
    o = run_model(c, b)
    check_ints(o, c.want, (name, backend))
    t = o["new_type"]
    assert ((o["new_assoc"] == -1) == ((t == 1) | (t == 3))).all(), "new_assoc = -1 exactly for types 1 and 3"
    assert o["new_pos"].shape == (o["n_new"], 3) and np.isfinite(o["new_pos"]).all()


def test_all_four_types_in_one_key_frame():
    assert sorted(cc.CASES["types_all_four"].want["new_type"].tolist()) == [1, 2, 3, 4]
    assert cc.CASES["types_all_four"].want["nb_stats"][0, 4] == 1, "and a rejected match"


def test_carry_case_differs_without_the_carry():
    c = cc.CASES["carry_created_feature_is_no_query"]
    o = run_model(c, numpy_ref, carry=False)
    assert any(np.asarray(o[k]).shape != np.asarray(c.want[k]).shape or (np.asarray(o[k]) != np.asarray(c.want[k])).any() for k in INT_KEYS), \
        "a batch of independent pairs gives the declared output: the case does not test the carry"


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_threshold_margin(name):
    assert cc.CASES[name].margins() > 1e-9, "an epipolar distance within a relative 1e-9 of its threshold: F's last bit could decide a match"


def test_baseline_cases_are_exact():
    for side, want in (("at", 0), ("ulp_below", 32), ("ulp_above", 0)):
        c = cc.CASES["baseline_" + side]
        d = c.ba["kf_twc"][1] - c.ba["kf_twc"][0]
        assert d[1] == 0 and d[2] == 0 and float(f32(d[0])) == d[0], "the norm is the float itself"
        assert (f32(d[0]) < f32(c.mb)) == bool(want)
    assert cc.CASES["baseline_at"].ba["kf_twc"][1][0] == cc.CASES["baseline_at"].mb


def _pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    if q[3] < 0:
        q = -q
    return np.concatenate([q, rng.uniform(-2, 2, 3)])


SEEDED_CAMS = (dict(cc.CAM), dict(fx=435.2, fy=431.7, cx=367.2, cy=252.2, bf=47.9, width=752, height=480))


def seeded_pairs(n=64, seed=5):
    rng = np.random.default_rng(seed)
    return [(_pose(rng), _pose(rng)) for _ in range(n)]


@pytest.mark.parametrize("ci", [0, 1])
def test_numpy_statement_against_synth(ci):
    """entrywise within 16 x 2^-53 x (|K^-T| |[t]x| |R12| |K^-1|): the forward-error bound of the product chain, evaluated with absolute
    values; the epipole within 2 float ulps"""
    cam = api.Camera(**SEEDED_CAMS[ci])
    fx, fy, cx, cy = ref.cam_scalars(SEEDED_CAMS[ci])
    Kinv = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1.0]])
    for p1, p2 in seeded_pairs():
        F, e = ref.fundamental_and_epipole(p1, p2, SEEDED_CAMS[ci])
        Fs, es = synth.fundamental_and_epipole(p1, p2, cam)
        R12 = synth.quat_to_R(p1[:4]) @ synth.quat_to_R(p2[:4]).T
        t12 = -(R12 @ p2[4:]) + p1[4:]
        sk = np.abs(np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]]))
        bound = 16 * 2.0 ** -53 * (np.abs(Kinv.T) @ sk @ np.abs(R12) @ np.abs(Kinv))
        assert (np.abs(F.reshape(3, 3) - Fs) <= bound).all(), (np.abs(F.reshape(3, 3) - Fs) / bound).max()
        assert (np.abs(e.astype(f64) - es.astype(f64)) <= 2 * np.spacing(np.abs(es)).astype(f64)).all(), (e, es)
