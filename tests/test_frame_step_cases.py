"""The two statements of the frame end and the hand-over - the sequential object model of tests/frame_step_ref.py and the vectorised
restatement of tests/frame_step_glue.py, which says what the device does - held to each other and to the DECLARED outputs of
tests/frame_step_cases.py: one case on each side of every decision.  No GPU; tests/test_gpu_frame_step.py runs the same cases on the
device."""
import numpy as np
import pytest

from tests import frame_step_cases as FC
from tests import frame_step_glue as G
from tests import frame_step_ref as R

F32 = np.float32


def poison_end(B, NF):
    return dict(held_mp=np.full((B, NF), -77, np.int32), held=np.full((B, NF), 77, np.uint8), stat=np.full((B, 8), -77, np.int32),
                ratio_map=np.full(B, -77.0, F32))


def check_end_case(out):
    """the declared outputs of FC.END on the outputs of one of the statements or of the device (poison: poison_end)"""
    for b, mode in enumerate(FC.END_MODES):
        assert out["stat"][b].tolist() == FC.END_STATS[b], b
        if mode == 2:  # lost: the bytes are kept
            assert (out["held_mp"][b] == -77).all() and (out["held"][b] == 77).all() and out["ratio_map"][b] == F32(-77.0)
            continue
        assert out["held_mp"][b].tolist() == FC.END_HELD_MP, b
        assert out["held"][b].tolist() == [int(r >= 0) for r in FC.END_HELD_MP], b
        assert out["ratio_map"][b].tobytes() == F32(FC.END_RATIO[b]).tobytes(), b


def test_the_float_facts_the_cases_rest_on():
    assert F32(3) / F32(10) == F32(0.3) and F32(1) / F32(5) == F32(0.2) and F32(7) / F32(20) == F32(0.35)
    assert F32(29) / F32(100) < F32(0.3) and F32(6) / F32(20) < F32(0.35) and F32(19) / F32(100) < F32(0.2)
    assert F32(80) * F32(0.25) == 20 and F32(80) * F32(0.75) == 60 and F32(84) * F32(0.75) == 63 and F32(80) * F32(0.4) == 32
    assert 33 < F32(84) * F32(0.4) < 34
    assert F32(FC.BELOW) < F32(FC.TH_DEPTH) < F32(FC.ABOVE) and np.nextafter(F32(FC.BELOW), F32(9)) == F32(FC.TH_DEPTH)


def test_end_case():
    m, ba = FC.small_map()
    a = FC.end_arrays()
    W = R.World(m, ba)
    ref = R.frame_end(m, ba, th_depth=FC.TH_DEPTH, rule=FC.END_RULE, world=W, poison=poison_end(4, len(FC.END)), **a)
    glue = G.frame_end(m, ba, th_depth=FC.TH_DEPTH, rule=FC.END_RULE, poison=poison_end(4, len(FC.END)), **a)
    check_end_case(ref)
    check_end_case(glue)
    # the frame's final is_outlier_ is the chain's array, byte for byte - carried through every statement by the model
    assert ref["is_outlier"].tobytes() == a["outlier"].tobytes()
    e = W.events
    assert e["cleared_flag_was_set"] == 0 and e["late_outlier"] == 0
    assert e["lost"] == 1 and e["tracked"] == 2 and e["tracked_by_keyframe"] == 1
    for k in ("temporal", "outlier_temporal", "outlier_row", "cleared_temporal", "cleared_row", "inlier_unobserved", "matched_local", "from_last"):
        assert e[k] >= 3, k


def test_end_without_last_observed_and_without_counts2():
    """NULL last_observed: every last-frame point observed, no temporal point - and no output changes; NULL counts2: every frame tracked"""
    m, ba = FC.small_map()
    a = dict(FC.end_arrays(), last_observed=None, counts2=None)
    W = R.World(m, ba)
    ref = R.frame_end(m, ba, th_depth=FC.TH_DEPTH, world=W, **a)
    glue = G.frame_end(m, ba, th_depth=FC.TH_DEPTH, **a)
    assert W.events["temporal"] == 0 and W.events["lost"] == 0
    for out in (ref, glue):
        assert out["stat"][:3].tolist() == [[1, 9, 4, 8, 0, 0, 0, 0]] * 3 and out["held_mp"][1].tolist() == FC.END_HELD_MP


@pytest.mark.parametrize("key", list(FC.COUNT))
def test_count_map_points(key):
    num_kfs, ref_kf = key
    m, ba = FC.small_map()
    a = FC.end_arrays()
    a["ref_kf"][:] = ref_kf
    rule = dict(FC.END_RULE, num_kfs=num_kfs)
    for out in (R.frame_end(m, ba, th_depth=FC.TH_DEPTH, rule=rule, **a), G.frame_end(m, ba, th_depth=FC.TH_DEPTH, rule=rule, **a)):
        assert out["stat"][[0, 2, 3], 4].tolist() == [FC.COUNT[key]] * 3 and out["stat"][1, 4] == 0


@pytest.mark.parametrize("name", list(FC.RULES))
def test_need_new_keyframe_at_its_thresholds(name):
    _, nmi, num_map, num_total, nref, verdict = FC.RULES[name]
    m, ba = FC.rule_map()
    a = FC.rule_frame(nmi, num_map, num_total)
    want = [1, nmi, num_map, num_total, nref, verdict, 0, 0]
    for out in (R.frame_end(m, ba, th_depth=FC.TH_DEPTH, rule=FC.rule_of(name), **a), G.frame_end(m, ba, th_depth=FC.TH_DEPTH, rule=FC.rule_of(name), **a)):
        assert out["stat"][0].tolist() == want, name
        assert out["ratio_map"][0].tobytes() == (F32(num_map) / F32(max(1, num_total))).tobytes()


def test_every_rule_has_its_other_side():
    """each threshold is met from both sides, and both verdict bits occur in every combination the reference can return"""
    v = {n: c[5] for n, c in FC.RULES.items()}
    for at, below in (("c1a_one_before", "c1a_at"), ("c1b_inliers_at", "c1b_inliers_below"), ("c1b_ratio_at", "c1b_ratio_below"),
                      ("c2_ref_at_kfs3", "c2_ref_below_kfs3"), ("c2_ref_at_kfs2", "c2_ref_below_kfs2"), ("c2_ref_at_kfs1", "c2_ref_below_kfs1"),
                      ("c2_map_at_300", "c2_map_below_300"), ("c2_map_at_301", "c2_map_below_301"), ("inliers_15", "inliers_16"),
                      ("c2_map_301_same_ratio", "c2_map_below_300")):
        assert v[at] == 0 and v[below] != 0, (at, below)
    assert set(v.values()) == {0, FC.NEED, FC.INTERRUPT, FC.NEED | FC.INTERRUPT}


@pytest.mark.parametrize("name", list(FC.REPLACE))
def test_note_replaced(name):
    steps, _ = FC.REPLACE[name]
    src, tgt = [s for s, _ in steps], [t for _, t in steps]
    none = -np.ones(FC.NMPCAP, np.int32)
    want = FC.replaced_array(name)
    assert np.array_equal(R.note_replaced(none, src, tgt), want) and np.array_equal(G.note_replaced(none, src, tgt), want)
    # the objects: Map::replaceMapPoint step by step (rows of the small map's table only)
    m, ba = FC.small_map()
    W = R.World(m, ba)
    W.note_replaced_steps(src, tgt)
    assert np.array_equal(W.mp_replaced(), np.where(want[:FC.NMP] < FC.NMP, want[:FC.NMP], -1))
    # an entry that is there already stays unless a step names its row; a device count cuts the list
    old = np.arange(FC.NMPCAP, dtype=np.int32)[::-1].copy()
    for n in (None, 0, 1, len(steps) + 3):
        r, g = R.note_replaced(old, src, tgt, n), G.note_replaced(old, src, tgt, n)
        assert np.array_equal(r, g), (name, n)
    assert np.array_equal(R.note_replaced(old, src, tgt, 0), old)


def next_args(held=None):
    m, ba = FC.after_map()
    tracked, prev = FC.next_poses()
    held = np.array([FC.NEXT_HELD if held is None else held] * 2, np.int32)
    return m, ba, tracked, prev, np.array([1, 2], np.int32), held


def check_next_rows(m, out, want):
    for b in range(out["held_mp"].shape[0]):
        rows = np.array(want["held_mp"])
        assert out["held_mp"][b].tolist() == want["held_mp"] and out["held"][b].tolist() == want["held"], b
        has = (rows >= 0) & (rows < FC.NMP)
        assert out["last_valid"][b].tolist() == has.astype(int).tolist()
        assert out["last_observed"][b].tolist() == [int(h == 1) for h in want["held"]]
        assert out["last_pt"][b].tobytes() == np.where(has[:, None], m["mp_pos"][np.where(has, rows, 0)], 0.0).tobytes()


def test_next_rows():
    m, ba, tracked, prev, ref_kf, held = next_args()
    rep = FC.replaced_array("all")
    fn = np.array([FC.NEXT_FEAT_NEW] * 2, np.int32)
    for f in (R.frame_next, G.frame_next):
        W = {"world": R.World(m, ba)} if f is R.frame_next else {}
        one = f(m, ba, tracked, prev, ref_kf, held, feat_new=fn, mp_base=FC.NEXT_MP_BASE, mp_replaced=rep, **W)
        check_next_rows(m, one, FC.NEXT_OUT)
        if W:
            e = W["world"].events
            assert e["stereo_new"] == 4 and e["stereo_nulled"] == 2 and e["replaced"] == 8 and e["held_unobserved"] == 6
        two = f(m, ba, tracked, prev, ref_kf, one["held_mp"], mp_replaced=rep)  # the chain A -> B -> C: B this frame, C the next
        check_next_rows(m, two, FC.NEXT_OUT_2)
        check_next_rows(m, f(m, ba, tracked, prev, ref_kf, held), FC.NEXT_PLAIN)
        assert (one["status"] == 0).all()


def test_next_rows_after_temporal_points():
    """a held == 2 slot that createTemporalPoints walks holds a temporal point afterwards: its last_mp is -1, not the row that was
    replaced or culled (tracking.cpp:441, :453)"""
    m, ba, tracked, prev, ref_kf, held = next_args()
    rep = FC.replaced_array("all")
    fn = np.array([FC.NEXT_FEAT_NEW] * 2, np.int32)
    depth = np.array([FC.NEXT_DEPTH] * 2, F32)
    W = R.World(m, ba)
    one = R.frame_next(m, ba, tracked, prev, ref_kf, held, feat_new=fn, mp_base=FC.NEXT_MP_BASE, mp_replaced=rep, world=W, feat_depth=depth, th_depth=FC.TH_DEPTH)
    check_next_rows(m, one, FC.NEXT_OUT)  # (the rows createTemporalPoints finds)
    flag, last_mp = G.temporal_last_mp(one["held_mp"], one["held"], depth, FC.TH_DEPTH)
    for b in range(2):
        assert one["temp_flag"][b].tolist() == flag[b].tolist() == FC.NEXT_TEMPORAL["temp_flag"]
        assert one["last_mp"][b].tolist() == last_mp[b].tolist() == FC.NEXT_TEMPORAL["last_mp"]
    e = W.events
    assert e["temporal_over_row"] == 4 and e["temporal_over_invalid_row"] == 2 and e["temporal_over_temporal"] == 0


def test_temporal_walk_break_keeps_the_rows_behind_it():
    """past 100 walked slots the first depth above th_depth ends the walk (:462): a held == 2 slot behind it keeps its row"""
    m, ba, tracked, prev, ref_kf, _ = next_args()
    NF = 130
    held = np.full((1, NF), 3, np.int32)  # (p3: valid, no observation - held == 2 everywhere)
    depth = np.linspace(1.0, 3.9, NF, dtype=F32)[None].copy()
    depth[0, 110:] = np.linspace(4.5, 9.0, NF - 110, dtype=F32)[::-1]  # (above th_depth, descending: index 129 is walked, then the break)
    out = R.frame_next(m, ba, tracked[:1], prev[:1], ref_kf[:1], held, feat_depth=depth, th_depth=FC.TH_DEPTH)
    flag, last_mp = G.temporal_last_mp(out["held_mp"], out["held"], depth, FC.TH_DEPTH)
    want = np.array([1] * 110 + [0] * 19 + [1], np.uint8)
    assert np.array_equal(out["temp_flag"][0], want) and np.array_equal(flag[0], want)
    assert np.array_equal(out["last_mp"][0], np.where(want != 0, -1, 3)) and np.array_equal(last_mp, out["last_mp"])


def test_next_malformed_rows_change_nothing():
    m, ba, tracked, prev, ref_kf, _ = next_args()
    rep = -np.ones(FC.NMPCAP, np.int32)
    for k, v in FC.BAD_REPLACED.items():
        rep[k] = v
    held = np.array([FC.BAD_HELD] * 2, np.int64).astype(np.int32)
    fn = np.array([FC.BAD_FEAT_NEW] * 2, np.int32)
    out = G.frame_next(m, ba, tracked, prev, ref_kf, held, feat_new=fn, mp_base=FC.BAD_MP_BASE, mp_replaced=rep)
    check_next_rows(m, out, FC.BAD_OUT)


def pose_bound(p):
    return 1e-12 * max(1.0, float(np.abs(np.asarray(p, np.float64)[4:]).max()))


def test_next_poses():
    """pose_prev NULL against given, a reference key-frame moved by a BA, a ref_kf outside the table; the fp64 statement against the
    model in extended precision within 1e-12 max(1, |t|) (the bound derived in tests/test_gpu_frame_step.py)"""
    m, ba, tracked, prev, ref_kf, held = next_args()
    LD = np.longdouble
    for pp in (None, prev):
        ref = R.frame_next(m, ba, tracked.astype(LD), None if pp is None else pp.astype(LD), ref_kf, held, dtype=LD)
        glue = G.frame_next(m, ba, tracked, pp, ref_kf, held)
        for b in range(2):
            for k in ("t_rc", "t_cr", "pose_lw", "pose_cw"):
                assert np.abs(glue[k][b] - ref[k][b]).max() <= pose_bound(ref[k][b]), (k, b)
            # T_c_r * Tcw(ref) is the tracked pose again, whatever the key-frame's pose
            assert np.abs(glue["pose_lw"][b] - R.se3_load(tracked[b])).max() <= pose_bound(tracked[b])
            if pp is None:
                assert glue["pose_cw"][b].tobytes() == glue["pose_lw"][b].tobytes()
            else:
                want = R.se3_mul(R.se3_mul(glue["pose_lw"][b], R.se3_inverse(R.se3_load(pp[b]))), glue["pose_lw"][b])
                assert glue["pose_cw"][b].tobytes() == want.tobytes() and np.abs(want - glue["pose_lw"][b]).max() > 1e-3
    moved = dict(ba, kf_pose=ba["kf_pose"].copy())
    moved["kf_pose"][1, 4:] += [0.01, -0.02, 0.03]  # the BA moved key-frame 1 between end and next
    a, b2 = G.frame_next(m, ba, tracked, prev, ref_kf, held), G.frame_next(m, moved, tracked, prev, ref_kf, held)
    assert np.abs(a["t_rc"][0] - b2["t_rc"][0]).max() > 1e-3 and a["t_rc"][1].tobytes() == b2["t_rc"][1].tobytes()
    assert np.abs(a["pose_lw"][0] - b2["pose_lw"][0]).max() <= 2 * pose_bound(tracked[0])
    poison = {k: np.full((2, 7), -77.0) for k in ("t_rc", "t_cr", "pose_lw", "pose_cw")}
    for bad in (-1, FC.NKF):
        out = G.frame_next(m, ba, tracked, prev, np.array([bad, 0], np.int32), held, poison=poison)
        ref = R.frame_next(m, ba, tracked, prev, np.array([bad, 0], np.int32), held)
        assert out["status"].tolist() == [R.BAD_REF, 0] and ref["status"].tolist() == [R.BAD_REF, 0]
        assert all((out[k][0] == -77.0).all() and (out[k][1] != -77.0).all() for k in poison)
        check_next_rows(m, out, FC.NEXT_PLAIN)  # (the rows do not depend on the poses)


# ---- the layers above the kernels
ENTRY_POINTS = ("gl_track_frame_end", "gl_map_note_replaced", "gl_track_frame_next")


def test_library_and_binding_table_hold_the_entry_points():
    from gmmloc_amd import _lib
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in lib._gl_signatures, name
    assert not lib._gl_missing


def test_binding_structs_follow_the_header():
    """every struct of the three calls: the ctypes fields are the header's members, in order"""
    import os
    import re
    from gmmloc_amd import _lib
    from tests.conftest import ROOT
    text = open(os.path.join(ROOT, "include", "gmmloc_hip.h")).read()
    for name in ("gl_frame_end_in", "gl_kf_rule", "gl_frame_end_out", "gl_frame_next_in", "gl_frame_next_out"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = [re.split(r"[\s\*]+", d.strip())[-1] for d in body.split(";") if d.strip()]
        assert members == [f for f, _ in getattr(_lib, name)._fields_], name


def test_python_layer_exports_the_wrappers():
    from gmmloc_amd import frame_step
    for name in ("frame_end", "note_replaced", "frame_next", "track_frame_step", "first_state", "kf_rule"):
        assert callable(getattr(frame_step, name)), name
    assert (frame_step.KF_NEED, frame_step.KF_INTERRUPT_BA, frame_step.FRAME_NEXT_BAD_REF) == (R.KF_NEED, R.KF_INTERRUPT_BA, R.BAD_REF)
