"""CPU: known answers for tests/local_map_ref.py, the restatement of Tracking::updateLocalMap (tracking.cpp:119-207) that
gl_update_local_map and gl_track_frame_chain_map are checked against; its two forms against each other; and the conditions on the
scenes of tests/test_gpu_local_map.py that keep those tests from passing vacuously."""
import numpy as np
import pytest

from gmmloc_amd import api, synth
from tests import local_map_ref as R
from tests import local_map_scenes as S
from tests import map_cases as MC


tiny_map, ROWS = MC.rows_map, MC.ROWS  # (the builder and the four key-frames of the hand-built cases: tests/map_cases.py)


def run(m, feat_mp, KFcap=8, NPcap=16, prev_kf=(6, 7), prev_mp=(9,), prev_ref=5):
    """both forms on one frame with sentinels behind the lists; they must agree"""
    lists = dict(local_kf=np.full((1, KFcap), -7, np.int32), n_local_kf=np.array([len(prev_kf)], np.int32), local_mp=np.full((1, NPcap), -7, np.int32),
                 n_local_mp=np.array([len(prev_mp)], np.int32), ref_kf=np.array([prev_ref], np.int32), status=np.array([-7], np.int32),
                 kf_count=np.full((1, m["kf_mp"].shape[0]), -7, np.int32))
    lists["local_kf"][0, :len(prev_kf)] = prev_kf
    lists["local_mp"][0, :len(prev_mp)] = prev_mp
    fa, a = R.update_local_map(m, np.array([feat_mp], np.int32), lists, R.frame_sets)
    fb, b = R.update_local_map(m, np.array([feat_mp], np.int32), lists, R.frame_vec)
    assert np.array_equal(fa, fb)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    return fa[0], {k: v[0] for k, v in a.items()}


def case(name):
    """the map and the frame of a case of tests/map_cases.py::LOCAL (which tests/test_gpu_map_cases.py runs on the device), through run()"""
    c = MC.LOCAL[name]
    a = c.args
    return run(c.m, a["feat_mp"], a["KFcap"], a["NPcap"], a["prev_kf"], a["prev_mp"], a["prev_ref"])


def test_point_held_by_two_features_counts_twice():
    assert MC.LOCAL["held_twice"].args["feat_mp"] == [0, 0, -1]
    fm, o = case("held_twice")  # point 0 (seen by kf 0 alone) held twice
    assert o["kf_count"].tolist() == [2, 0, 0, 0] and o["ref_kf"] == 0 and o["status"] == 0
    assert o["local_kf"][:o["n_local_kf"]].tolist() == [0] and o["local_mp"][:o["n_local_mp"]].tolist() == [0, 1, 2]
    assert o["local_kf"][1:].tolist() == [7] + [-7] * 6 and o["local_mp"][3:].tolist() == [-7] * 13  # (what lay behind the lists stays)


def test_invalid_held_point_is_cleared_and_counts_nothing():
    c = MC.LOCAL["invalid_held_point"]
    assert c.m["mp_valid"].tolist() == [1, 0, 1, 1, 1, 1, 1] and c.args["feat_mp"] == [1, 4, -1, 1]
    fm, o = case("invalid_held_point")  # point 1 is invalid: both features lose it; point 4 is seen by kf 2
    assert fm.tolist() == [-1, 4, -1, -1]
    assert o["kf_count"].tolist() == [0, 0, 1, 0] and o["ref_kf"] == 2
    assert o["local_mp"][:o["n_local_mp"]].tolist() == [4]  # kf 2 holds 4 and the invalid 1


def test_invalid_key_frame_is_counted_but_neither_local_nor_reference():
    c = MC.LOCAL["invalid_key_frame"]
    assert c.m["kf_valid"].tolist() == [1, 0, 1, 1] and c.args["feat_mp"] == [1, 2, 3]
    fm, o = case("invalid_key_frame")  # kf 1 sees all three (count 3), kf 0 sees 1 and 2, kf 2 sees 1
    assert o["kf_count"].tolist() == [2, 3, 1, 0]
    assert o["ref_kf"] == 0 and o["local_kf"][:o["n_local_kf"]].tolist() == [0, 2]
    assert o["local_mp"][:o["n_local_mp"]].tolist() == [0, 1, 2, 4]  # point 3 is held by the invalid key-frame alone


def test_all_counted_key_frames_invalid_empties_the_lists_and_keeps_the_reference():
    c = MC.LOCAL["all_counted_invalid"]
    assert c.m["kf_valid"].tolist() == [1, 1, 1, 0] and c.args["feat_mp"] == [5, 6]
    fm, o = case("all_counted_invalid")
    assert o["kf_count"].tolist() == [0, 0, 0, 2] and o["status"] == 0
    assert o["n_local_kf"] == 0 and o["n_local_mp"] == 0 and o["ref_kf"] == 5
    assert o["local_kf"].tolist() == [6, 7] + [-7] * 6 and o["local_mp"].tolist() == [9] + [-7] * 15  # (nothing written)


def test_empty_counter_keeps_everything():
    c = MC.LOCAL["empty_counter"]  # points 7, 8: no observation (temporal points)
    assert c.m["kf_mp"].tolist() == ROWS + [[-1, -1, -1, -1]] and len(c.m["obs_ptr"]) == 10 and c.args["feat_mp"] == [-1, 7, -1, 8]
    fm, o = case("empty_counter")
    assert fm.tolist() == [-1, 7, -1, 8] and o["status"] == R.KEPT
    assert o["kf_count"].tolist() == [0] * 5
    assert o["n_local_kf"] == 2 and o["n_local_mp"] == 1 and o["ref_kf"] == 5
    assert o["local_kf"].tolist() == [6, 7] + [-7] * 6 and o["local_mp"].tolist() == [9] + [-7] * 15
    assert MC.LOCAL["holds_nothing"].args["feat_mp"] == [-1, -1]
    fm, o = case("holds_nothing")
    assert o["status"] == R.KEPT and o["ref_kf"] == 5


def test_tie_goes_to_the_lowest_row():
    assert MC.LOCAL["tie_lowest_row"].args["feat_mp"] == [1]
    fm, o = case("tie_lowest_row")  # point 1: kf 0, 1, 2 with one count each
    assert o["kf_count"].tolist() == [1, 1, 1, 0] and o["ref_kf"] == 0
    c = MC.LOCAL["tie_lowest_valid_row"]
    assert c.m["kf_valid"].tolist() == [0, 1, 1, 1] and c.args["feat_mp"] == [1, 4, 3]
    fm, o = case("tie_lowest_valid_row")  # kf 1: points 1, 3; kf 2: points 1, 4; kf 0 (invalid): point 1
    assert o["kf_count"].tolist() == [1, 2, 2, 0] and o["ref_kf"] == 1


def test_null_and_invalid_points_of_a_key_frame_are_left_out_and_a_shared_point_is_listed_once():
    c = MC.LOCAL["shared_point_once"]
    assert c.m["mp_valid"].tolist() == [1, 1, 0, 1, 1, 1, 1] and c.args["feat_mp"] == [1]
    fm, o = case("shared_point_once")  # local: kf 0, 1, 2 - point 1 is in all three, point 2 (invalid) in two, nulls in each
    assert o["local_kf"][:o["n_local_kf"]].tolist() == [0, 1, 2]
    assert o["local_mp"][:o["n_local_mp"]].tolist() == [0, 1, 3, 4]


def test_truncation_keeps_the_lowest_rows_and_reports_the_true_counts():
    c = MC.LOCAL["truncated_both"]
    assert (c.args["feat_mp"], c.args["KFcap"], c.args["NPcap"]) == ([1], 2, 3)
    fm, o = case("truncated_both")
    assert o["n_local_kf"] == 3 and o["n_local_mp"] == 5
    assert o["local_kf"].tolist() == [0, 1] and o["local_mp"].tolist() == [0, 1, 2]
    assert o["status"] == R.MP_TRUNCATED | R.KF_TRUNCATED
    c = MC.LOCAL["truncated_points"]
    assert (c.args["feat_mp"], c.args["KFcap"], c.args["NPcap"]) == ([1], 3, 4)
    fm, o = case("truncated_points")
    assert o["status"] == R.MP_TRUNCATED and o["local_kf"].tolist() == [0, 1, 2]


def test_malformed_rows_are_skipped():
    m = tiny_map(ROWS, 7)
    m["kf_mp"][0, 2] = 99  # a key-frame slot outside the map
    m["obs_kf"] = m["obs_kf"].copy()
    first_of_5 = m["obs_ptr"][5]
    m["obs_kf"][first_of_5] = 44  # point 5's only observation names no key-frame
    fm, o = run(m, [0, 77, -3, 5])
    assert fm.tolist() == [0, 77, -3, 5] and o["kf_count"].tolist() == [1, 0, 0, 0]
    assert o["local_mp"][:o["n_local_mp"]].tolist() == [0, 1, 2]
    m["obs_ptr"] = m["obs_ptr"].copy()
    m["obs_ptr"][1] = 1000  # point 0's range leaves the CSR
    fm, o = run(m, [0])
    assert o["status"] == R.KEPT


def test_gather_and_index_tables():
    m = tiny_map(ROWS, 7)
    m.update(mp_pos=np.arange(21.0).reshape(7, 3), mp_normal=-np.arange(21.0).reshape(7, 3), mp_max_dist=np.arange(7, dtype=np.float32) + 10,
             mp_min_dist=np.arange(7, dtype=np.float32), mp_desc=np.arange(7 * 32).reshape(7, 32).astype(np.uint8))
    g = R.gather_local_map(m, np.array([1, 3, 4, 6, -7]), 4, 6, [4, -1, 0, 6, 1], [3, 5])
    assert g["mp_cand"].tolist() == [1, 1, 1, 1, 0, 0] and g["mp_pos"][:, 0].tolist() == [3, 9, 12, 18, 0, 0]
    assert g["mp_max_dist"].tolist() == [11, 13, 14, 16, 0, 0] and g["mp_desc"][1, 0] == 96 and not g["mp_desc"][4:].any()
    assert g["last_to_local"].tolist() == [2, -1, -1, 3, 0] and g["kf_to_local"].tolist() == [1, -1]
    g = R.gather_local_map(m, np.array([1, 3, 4, 6]), 4, 2, [4, 3], None)  # a list cut at two slots
    assert g["mp_cand"].tolist() == [1, 1] and g["last_to_local"].tolist() == [-1, 1]


def test_derive_feat_mp_clears_an_invalid_point_in_full():
    m = tiny_map(ROWS, 7, mp_valid=[1, 1, 0, 1, 1, 1, 1])
    fm, ml, mk = R.derive_feat_mp(m, [0, -1, 2, -1, 1], [-1, 1, -1, 0, -1], [1, 2, -1], [2, 5], 0)
    assert fm.tolist() == [1, 5, -1, -1, -1]  # feature 2 holds a temporal point, 3 and 4 the invalid point 2
    assert ml.tolist() == [0, -1, 2, -1, -1] and mk.tolist() == [-1, 1, -1, -1, -1]
    fm, ml, mk = R.derive_feat_mp(m, [0, -1], [-1, 1], [1], [2, 5], 2)  # a lost frame holds nothing
    assert fm.tolist() == [-1, -1] and ml.tolist() == [0, -1]


@pytest.mark.parametrize("name", ["tiny", "small", "kf_over_bound"])
def test_both_forms_agree_on_synthetic_maps(name):
    m, feat_mp, lists = S.update_scene(name)
    fa, a = R.update_local_map(m, feat_mp, lists, R.frame_sets)
    fb, b = R.update_local_map(m, feat_mp, lists, R.frame_vec)
    assert np.array_equal(fa, fb)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_synthetic_map_is_consistent_and_leaves_earlier_seeds_alone():
    cam = api.Camera()
    before = synth.synth_chain_frame(64, 64, 64, 4800, cam)
    s = synth.synth_chain_map([synth.synth_chain_frame(64, 64, 64, 4800, cam)], 3, 400, 60, 30)
    after = synth.synth_chain_frame(64, 64, 64, 4800, cam)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    m = s["map"]
    pt = np.repeat(np.arange(400), np.diff(m["obs_ptr"]))
    kk, ss = np.nonzero(m["kf_mp"] >= 0)
    assert sorted(zip(pt.tolist(), m["obs_kf"].tolist())) == sorted(zip(m["kf_mp"][kk, ss].tolist(), kk.tolist()))
    assert len(set(zip(pt.tolist(), m["obs_kf"].tolist()))) == len(pt)  # a key-frame sees a point once
    assert np.array_equal(m["mp_pos"][s["rows"][0]], before["mp_pos"]) and np.array_equal(m["mp_desc"][s["rows"][0]], before["mp_desc"])
    has = before["last_to_local"] >= 0
    assert np.array_equal(s["last_mp"][0][has], s["rows"][0][before["last_to_local"][has]])


@pytest.mark.parametrize("name", S.BATCHED)
def test_update_scenes_hold_every_kind_of_frame(name):
    """every batch of tests/test_gpu_local_map.py holds a frame whose list changes, one with a cleared held point, one with an invalid
    key-frame that was counted, one with a tie for the reference key-frame and one with an empty counter; nothing is truncated (the
    truncation test cuts the capacities itself)"""
    m, feat_mp, lists = S.update_scene(name)
    kinds = S.frame_kinds(m, feat_mp, lists)
    for k, v in kinds.items():
        assert v.any(), k
    fm, out = R.update_local_map(m, feat_mp, lists)
    assert ((out["status"] & ~R.KEPT) == 0).all()
    assert out["n_local_mp"].max() > lists["local_mp"].shape[1] // 8


@pytest.mark.parametrize("name", list(S.CHAIN_SCENES))
def test_chain_scenes_match_something_in_every_tracked_frame(oracle, name):
    """the reference sequence (oracle front -> restatement -> gather -> oracle stage 3) on the chain scenes: the frames take the paths
    their scene is named for, every frame that is not lost finds local map points in stage 3, every tracked frame's list is new and
    fits NPcap with little to spare, and (but for the scenes without invalid points) some held point is cleared"""
    cam = api.Camera()
    frames, s, lists, KFcap, NPcap = S.chain_scene(name)
    cleared = 0
    for b, f in enumerate(frames):
        n3, h, r = S.oracle_sequence(oracle, cam, f, b, s, lists)
        assert r["mode"] == S.CHAIN_MODES[name][b]
        st = int(h["lists"]["status"][0])
        if r["mode"] == 2:
            assert st == R.KEPT and np.array_equal(h["lists"]["local_mp"][0], lists["local_mp"][b])
            continue
        assert st == 0 and n3 > 0, (b, st, n3)
        n = int(h["lists"]["n_local_mp"][0])
        assert n <= NPcap and n > NPcap // 2, (b, n, NPcap)
        assert not np.array_equal(h["lists"]["local_mp"][0], lists["local_mp"][b])
        held_before = R.derive_feat_mp(dict(s["map"], mp_valid=None), r["match_last"], r["match_kf"], s["last_mp"][b], s["kf_feat_mp"][b], r["mode"])[0]
        cleared += int(((held_before >= 0) & (h["feat_mp"] < 0)).sum())
    assert (cleared > 0) == (name not in S.WITHOUT_INVALID_POINTS)
