"""The checker of tests/test_gpu_map_stats.py checked on the CPU: the hand-built cases of tests/map_stats_cases.py give their DECLARED
outputs on the sequential model of tests/map_stats_ref.py; removeMapPoints judged on a SNAPSHOT with the first-occurrence rule equals
the sequential walk with real list erasure and real Map::removeMapPoint calls - the fact gl_cull_map_points rests on -; every branch
ran; the library, the binding table and the Python layer hold the five entry points."""
import numpy as np
import pytest

from tests import map_edit_ref as E
from tests import map_edit_scenes as ES
from tests import map_stats_cases as SC
from tests import map_stats_ref as R

ENTRY_POINTS = ("gl_map_stats_track", "gl_map_stats_new_points", "gl_map_cand_append", "gl_map_stats_merge", "gl_cull_map_points")


def cull_model(variant, cand):
    sc = SC.cull_scene(variant)
    return R.Model(sc["m"], sc["ba"]).set_stats(sc["visible"], sc["found"], sc["ref_idx"], sc["kf_idx"], cand), sc


@pytest.mark.parametrize("variant", ["rows", "shifted"])
@pytest.mark.parametrize("name", list(SC.LISTS))
def test_cull_cases_give_their_declared_outputs(name, variant):
    cand, verdict, kept, rm = SC.LISTS[name]
    M, sc = cull_model(variant, cand)
    v_snap, kept_snap, rm_snap = M.judge_snapshot(SC.KF_ROW)
    v, removed = M.remove_map_points(SC.KF_ROW)
    assert v == verdict and M.cand == kept and removed == rm, (name, v, M.cand, removed)
    assert (v_snap, kept_snap, rm_snap) == (verdict, kept, rm), name
    assert (M.events["bad_row"] > 0) == (name in SC.BAD_ROW_LISTS)
    # what the composite leaves: the sequential removals are gl_map_remove(rm_mp) of the list
    rows, _ = E.map_remove(sc["m"], sc["ba"], rm_mp=rm)
    got = M.to_rows()
    for k in ("mp_valid", "kf_mp", "obs_ptr", "obs_kf", "obs_feat"):
        assert np.array_equal(got[k], rows[k]), (name, k)


def test_every_point_of_the_table_has_its_declared_verdict_alone():
    for i, p in enumerate(SC.POINTS):
        M, _ = cull_model("rows", [i])
        v, removed = M.remove_map_points(SC.KF_ROW)
        assert v == [p[6]], (p[0], v)
        assert removed == ([i] if p[6] in (R.RATIO, R.YOUNG_FEW) else []) and M.cand == ([i] if p[6] == R.KEPT else [])


def test_the_table_stands_on_both_sides_of_every_decision():
    """what the names say: the weights and ages the model sees, and the float32 facts of the ratio rows"""
    M, sc = cull_model("rows", [])
    w = {p[0]: M.points[i].num_obs for i, p in enumerate(SC.POINTS)}
    assert w["age2_weight3_stereo_mono"] == w["age2_weight3_three_mono"] == w["age1_weight3"] == w["age3_weight3"] == 3
    assert w["age2_weight4_two_stereo"] == w["age2_weight4_four_mono"] == w["age3_weight4_four_mono"] == 4 and w["age3_weight5"] == 5
    q = np.float32(0.25)
    assert R.found_ratio(1, 4) == q and R.found_ratio(1, 5) < q and R.found_ratio(4194303, 16777212) == q
    assert R.found_ratio(4194304, 16777217) == q and 4194304 * 4 < 16777217  # kept by the rounding of visible alone
    assert R.found_ratio(4194304, 16777218) == np.float32(0.24999997) < q
    assert np.float32(16777219) == np.float32(2 ** 24 + 4) and R.found_ratio(4194304, 16777219) < q and R.found_ratio(8388607, 33554431) < q
    assert np.isnan(R.found_ratio(0, 0)) and np.isinf(R.found_ratio(1, 0))
    assert not R.found_ratio(0, 0) < q and not R.found_ratio(1, 0) < q


def test_wide_case_needs_the_64_bit_subtraction():
    cand, verdict, kept, rm = SC.WIDE_LIST
    M, sc = cull_model("wide", cand)
    v, removed = M.remove_map_points(SC.KF_ROW)
    assert v == verdict and M.cand == kept and removed == rm
    curr, ref = np.int32(SC.WIDE_KF_IDX[SC.KF_ROW]), np.int32(SC.WIDE_POINTS[0][0])
    with np.errstate(over="ignore"):
        assert int(curr - ref) == -1  # what 32 bits make of it: "kept"


def test_snapshot_verdicts_equal_the_sequential_walk():
    """a few hundred random lists with duplicates on the scenes of tests/map_edit_scenes.py"""
    events = None
    for name, count in (("tiny", 300), ("small", 12)):
        sc = ES.scene(name)
        base = R.Model(sc["m"], sc["ba"])
        for i in range(count):
            rng = np.random.default_rng(1000 * count + i)
            c = SC.random_case(sc, rng, int(rng.integers(0, 60)))
            M = R.Model(sc["m"], sc["ba"]) if i else base
            M.set_stats(c["visible"], c["found"], c["ref_idx"], c["kf_idx"], c["cand"])
            snap = M.judge_snapshot(c["kf_row"])
            v, removed = M.remove_map_points(c["kf_row"])
            assert (v, M.cand, removed) == snap, (name, i)
            assert len(set(removed)) == len(removed)
            rows, _ = E.map_remove(sc["m"], sc["ba"], rm_mp=removed)
            got = M.to_rows()
            for k in ("mp_valid", "kf_mp", "obs_ptr", "obs_kf", "obs_feat"):
                assert np.array_equal(got[k], rows[k]), (name, i, k)
            events = M.events if events is None else events + M.events
    for k in ("kept", "invalid", "invalid_again", "ratio", "young_few", "aged", "bad_row", "kept_nan_inf"):
        assert events[k] > 0, (k, dict(events))


def test_track_case_gives_its_declared_outputs():
    t, a = SC.TRACK, SC.track_arrays()
    ones = np.ones(t["NMP"], np.int32)
    vis, fnd = R.track(ones, ones, t["NMP"], **a)
    assert vis.tolist() == t["visible_out"] and fnd.tolist() == t["found_out"]
    m, ba = SC.build_map([(1, ())] * t["NMP"])
    M = R.Model(m, ba)
    R.model_track(M, **a)
    assert M.num_visible == t["visible_out"] and M.num_found == t["found_out"]
    ev = M.events
    assert ev["lost"] == 1 and ev["held_twice"] == 1 and ev["in_view"] == 4 and ev["matched_local"] == 3 and ev["outlier"] == 3 and ev["found"] == 6


def test_tracker_statements_on_invalid_temporal_and_seen_points():
    """the branches the chain's outputs cannot reach: a held INVALID point is un-held and counts nothing, a temporal point has no
    counter, a local point the frame holds (or has dropped) is not counted a second time"""
    m, ba = SC.build_map([(1, ()), (0, ()), (1, ()), (1, ()), (0, ())])
    M = R.Model(m, ba)
    frame = [0, 1, R.TEMPORAL, -1]
    M.search_local_points_stats(frame, [0, 2, 3, 4], [1, 1, 1, 1], seen=(3,))
    assert frame == [0, -1, R.TEMPORAL, -1] and M.num_visible == [2, 1, 2, 1, 1]
    M.track_local_map_stats(frame, [0, 0, 0, 0])
    assert M.num_found == [2, 1, 1, 1, 1] and frame == [0, -1, R.TEMPORAL, -1]
    M.track_local_map_stats(frame, [1, 0, 1, 0])
    assert M.num_found == [2, 1, 1, 1, 1] and frame == [-1, -1, -1, -1]
    assert M.events["held_invalid"] == 1 and M.events["held_temporal"] == 1


def test_merge_case_gives_its_declared_outputs():
    c = SC.MERGE
    vis, fnd = R.merge(c["visible"], c["found"], c["NMP"], c["src"], c["tgt"])
    assert vis.tolist() == c["visible_out"] and fnd.tolist() == c["found_out"]
    # and on the model: replaceMapPoint with its counters, the rows outside the table skipped as the call skips them
    m, ba = SC.build_map([(1, ())] * c["NMP"])
    M = R.Model(m, ba).set_stats(c["visible"], c["found"], [-1] * c["NMP"])
    for s, t in zip(c["src"], c["tgt"]):
        if 0 <= s < c["NMP"] and 0 <= t < c["NMP"]:
            M.replace_map_point(M.points[s], M.points[t])
    assert M.num_visible == c["visible_out"] and M.num_found == c["found_out"]
    assert M.events["replace_self"] == 1 and M.events["replace"] == 6


def test_new_point_takes_the_key_frames_idx():
    m, ba = SC.build_map([(1, ())] * 2)
    M = R.Model(m, ba).set_stats([5, 5], [5, 5], [0, 0], kf_idx=[10, 11, 13, 14, 17, 18, 20, 21])
    for k in (2, -1, SC.NKF):
        M.new_point(k)
    assert M.num_visible == [5, 5, 1, 1, 1] and M.num_found == [5, 5, 1, 1, 1] and M.ref_idx == [0, 0, 13, -1, -1]


def test_library_and_binding_table_hold_the_entry_points():
    from gmmloc_amd import _lib
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in lib._gl_signatures, name
    assert not lib._gl_missing
    fields = [f for f, _ in _lib.gl_map_stats._fields_]
    assert fields == ["mp_visible", "mp_found", "mp_ref_idx", "kf_idx", "cand", "n_cand", "cand_cap", "reserved_"]


def test_python_layer_exports_the_wrappers():
    from gmmloc_amd import map_stats
    for name in ("map_stats_alloc", "map_stats_track", "map_stats_new_points", "map_cand_append", "map_stats_merge", "cull_map_points",
                 "track_frame_with_stats", "remove_map_points_from_map"):
        assert callable(getattr(map_stats, name)), name
