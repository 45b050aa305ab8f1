"""CPU: known answers for tests/map_point_ref.py, the restatement of MapPoint::computeDistinctiveDescriptors (mappoint.cpp:126-190) and
MapPoint::updateNormalAndDepth (:211-255) that gl_update_map_points is checked against.  The descriptors are prefix masks (the first b
bits set), so that two of them are |b1 - b2| apart and every median can be worked out by hand."""
import numpy as np

from gmmloc_amd import synth
from tests import map_cases as MC
from tests import map_point_ref as M

NKF, NFK = MC.PT_NKF, MC.PT_NFK
prefix, table, points, sentinel, with_descs = MC.prefix, MC.table, MC.points, MC.sentinel, MC.with_descs  # (the builders: tests/map_cases.py)


def run(kf, mp, what=3):
    """both forms of the restatement; they must agree byte for byte"""
    NP = len(mp["obs_ptr"]) - 1
    a, b = sentinel(NP), sentinel(NP)
    for p in range(NP):
        M.refresh_point(kf, mp, p, a, what)
    M.update_map_points_ref(kf, mp, b, what)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    return a


def case(name, what=3):
    """the key-frame table and the points of a case of tests/map_cases.py::POINTS (which tests/test_gpu_map_cases.py runs on the device)"""
    c = MC.POINTS[name]
    return run(c.m, c.ba, what)


def test_n1_n2_first_valid_observation():
    o = case("n1_n2")
    assert (o["desc"][0] == prefix(5)).all()
    assert (o["desc"][1] == prefix(50)).all()  # medians 0 and 41: element (2-1)/2 = 0 of each sorted row -> both 0, the first wins
    assert (o["desc"][2] == prefix(9)).all()


def test_n3_and_n4_hand_medians():
    # N = 3, bits 0 / 10 / 6: rows {0,10,6} {10,0,4} {6,4,0}, element 1 of the sorted rows 6 / 4 / 4 -> row 1 (the first 4)
    # N = 4, bits 0 / 20 / 8 / 9: rows sorted {0,8,9,20} {0,11,12,20} {0,1,8,12} {0,1,9,11}, element 1: 8 / 11 / 1 / 1 -> row 2
    o = case("n3_n4")
    assert (o["desc"][0] == prefix(10)).all()
    assert (o["desc"][1] == prefix(8)).all()
    kf = MC.POINTS["n3_n4"].m
    assert all((kf["desc"][k, 0] == prefix(b)).all() for k, b in enumerate((0, 10, 6, 0, 20, 8, 9)))
    assert M.distinctive_index(np.array([prefix(b) for b in (0, 10, 6)])) == 1
    assert M.distinctive_index(np.array([prefix(b) for b in (0, 20, 8, 9)])) == 2


def test_median_tie_first_row_wins():
    # bits 0 / 10 / 4: element 1 of the sorted rows {0,4,10} {0,6,10} {0,4,6} = 4 / 6 / 4: rows 0 and 2 tie, row 0 wins
    assert M.distinctive_index(np.array([prefix(b) for b in (0, 10, 4)])) == 0
    assert (case("median_tie")["desc"][0] == prefix(0)).all() and (MC.POINTS["median_tie"].m["desc"][2, 0] == prefix(4)).all()
    # five descriptors, the first one bit away from the other four: its median is 1, rows 1 .. 4 have 0 -> row 1
    d = np.array([prefix(3)] * 5)
    d[0, 31] = 1
    assert M.distinctive_index(d) == 1


def test_invalid_keyframes_skipped_in_descriptor_counted_in_normal():
    c = MC.POINTS["invalid_kf_skipped"]
    assert c.m["valid"].tolist() == [0] + [1] * 7 and c.ba["ref_kf"].tolist() == [1] and c.ba["obs_kf"].tolist() == [0, 1, 2, 3]
    o = case("invalid_kf_skipped")
    assert (o["desc"][0] == prefix(10)).all()  # the N = 3 case above on kf 1 .. 3
    # with kf 0: bits 7 / 0 / 10 / 6, element 1 of the sorted rows {0,1,3,7} {0,6,7,10} {0,3,4,10} {0,1,4,6} = 1 / 6 / 3 / 1 -> row 0
    assert MC.POINTS["invalid_kf_valid"].m["valid"].all()
    assert (case("invalid_kf_valid")["desc"][0] == prefix(7)).all()
    # normal: kf 0 (1,0,0) -> (-1,0,0); kf 1 (0,-3,0) -> (0,1,0); kf 2 (0,0,-4) -> (0,0,1); kf 3 (4,0,0) -> (-1,0,0); over n = 4
    assert o["normal"][0].tolist() == [-0.5, 0.25, 0.25]
    assert o["max_dist"][0] == np.float32(3.0)  # |pos - Ow_ref| = 3, octave of feature 0 = 0
    assert o["min_dist"][0] == np.float32(np.float32(3.0) / M.scale_factors()[7])


def test_ref_keyframe_not_observed_uses_feature_zero():
    c = MC.POINTS["ref_not_observed"]
    assert c.m["oct"][5].tolist() == [6, 2, 2, 2] and c.ba["ref_kf"].tolist() == [5] and c.args["what"] == 2
    o = case("ref_not_observed", what=2)
    sf = M.scale_factors()
    d = np.float32(6.0)  # kf 5 at (6, 0, 0)
    assert o["max_dist"][0] == np.float32(d * sf[6])
    assert o["min_dist"][0] == np.float32(np.float32(d * sf[6]) / sf[7])
    assert (o["desc"] == 0xA5).all()  # what = 2: the descriptor is not written
    # observed: the ref key-frame's own observation decides (feature 3 -> octave 3)
    assert MC.POINTS["ref_observed"].ba["ref_kf"].tolist() == [1]
    o = case("ref_observed", what=2)
    assert o["max_dist"][0] == np.float32(np.float32(3.0) * sf[3])


def test_point_at_camera_centre_adds_zero():
    o = case("at_camera_centre", what=2)  # kf 7 sits on the point
    assert o["normal"][0].tolist() == [0.0, 0.5, 0.0]
    o = case("only_at_camera_centre", what=2)
    assert o["normal"][0].tolist() == [0.0, 0.0, 0.0] and o["max_dist"][0] == 0.0 and o["min_dist"][0] == 0.0


def test_octave_7():
    assert MC.POINTS["octave_7"].m["oct"][2, 1] == 7
    o = case("octave_7", what=3)  # 5 from kf 2 at (0, 0, -4)
    sf = M.scale_factors()
    assert o["max_dist"][0] == np.float32(np.float32(5.0) * sf[7])
    assert o["min_dist"][0] == np.float32(o["max_dist"][0] / sf[7])
    assert o["normal"][0].tolist() == [0.0, 0.0, 1.0]
    assert MC.POINTS["octave_8"].m["oct"][2, 1] == 8  # outside 0 .. 7: normal and depth untouched, the descriptor still written
    o = case("octave_8", what=3)
    assert (o["normal"] == -7.0).all() and o["max_dist"][0] == -1.0 and (o["desc"][0] == 0).all()


def test_untouched_points():
    kf = with_descs(table(), [(0, 0, 4), (1, 0, 8)])
    rows = [[(0, 0), (1, 0)]] * 3 + [[]] + [[(0, 0), (9, 0)], [(0, 0), (1, 7)], [(0, -1)]]
    mp = points(rows, ref=[0, 0, 99, 0, 0, 0, 0], valid=[1, 0, 1, 1, 1, 1, 1])
    o = run(kf, mp)
    assert (o["desc"][0] == prefix(4)).all() and o["max_dist"][0] == np.float32(1.0)
    assert (o["desc"][1:2] == 0xA5).all() and (o["normal"][1] == -7.0).all()       # invalid point
    assert (o["desc"][2] == prefix(4)).all() and o["max_dist"][2] == -1.0           # ref_kf out of range: descriptor only
    assert (o["desc"][3:] == 0xA5).all() and (o["max_dist"][3:] == -1.0).all()      # no observations, bad key-frame / feature
    mp["obs_ptr"][1] = 9  # a row past NOBS, and the next one runs backwards
    o = run(kf, mp)
    assert (o["desc"][:2] == 0xA5).all() and (o["max_dist"][:2] == -1.0).all()


def test_batched_equals_sequential_on_a_synthetic_map():
    m = synth.synth_map_points(1500, 7)
    assert len(set(np.diff(m["mp"]["obs_ptr"]).tolist())) > 20
    run(m["kf"], m["mp"])
    m = synth.synth_map_points(8, 8, NKF=401, counts=[0, 1, 2, 3, 33, 64, 65, 300])
    o = run(m["kf"], m["mp"])
    assert (o["desc"][0] == 0xA5).all() and (o["desc"][1:] != 0xA5).any(1).all()
