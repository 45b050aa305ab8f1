"""CPU: every case of tests/map_cases.py gives its DECLARED output under both forms of its restatement - connections_seq / _vec,
window_seq / _vec, Model / cull_by_state, Model.map_remove, frame_sets / frame_vec, refresh_point / update_map_points_ref - so that
tests/test_gpu_map_cases.py can hold the device to the declaration alone; the two cases of every DECISIONS pair differ in the declared
outputs and the inputs the table names, and in nothing else; the descriptor sets and the structural cases meet the conditions they
were built for."""
import numpy as np
import pytest

from tests import ba_window_ref as R
from tests import ba_window_scenes as S
from tests import local_map_ref as L
from tests import map_cases as MC
from tests import map_edit_ref as E
from tests import map_point_ref as MP


def same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, a.ravel()[:16], b.ravel()[:16])


@pytest.mark.parametrize("form", [R.connections_seq, R.connections_vec], ids=["seq", "vec"])
@pytest.mark.parametrize("name", list(MC.CONN))
def test_connections_case(name, form):
    c = MC.CONN[name]
    NKF = c.m["kf_mp"].shape[0]
    same(R.update_connections(c.m, [c.args["kf"]], MC.conn_out(c.args["Ccap"], NKF), form), MC.conn_arrays(c), name)


@pytest.mark.parametrize("form", [R.window_seq, R.window_vec], ids=["seq", "vec"])
@pytest.mark.parametrize("name", list(MC.WINDOW))
def test_window_case(name, form):
    c = MC.WINDOW[name]
    o = c.out
    assert o["sizes"] == [len(o["free"]), len(o["fixed"]), len(o["pts"]), sum(len(l) for l in o["obs"])] and len(o["obs"]) == len(o["pts"])
    slab = MC.empty_slab(c.args["caps"])
    ref = S.empty_slab(1, c.args["caps"])
    assert all(slab[k].dtype == ref[k].dtype and np.array_equal(slab[k], ref[k]) for k in ref)  # (the same sentinels as the random scenes)
    got, _ = R.ba_window_build(c.m, c.ba, [c.args["kf"]], slab, form)
    same(got, MC.window_arrays(c), name)


@pytest.mark.parametrize("form", ["model", "by_state"])
@pytest.mark.parametrize("name", list(MC.CULL))
def test_cull_case(name, form):
    c = MC.CULL[name]
    cand, n_cand, want = MC.cull_arrays(c)
    d, th = c.args["kf_depth"], c.args["th_depth"]
    judge = None if form == "model" else (lambda lst: E.cull_by_state(c.m, c.ba, lst, d, th))
    same(E.cull_keyframes(c.m, c.ba, cand, n_cand, d, th, MC.cull_out(cand.shape[1]), judge), want, name)


@pytest.mark.parametrize("name", list(MC.REMOVE))
def test_remove_case(name):
    c = MC.REMOVE[name]
    a = c.args
    rows, status = E.map_remove(c.m, c.ba, a["rm_mp"], a["erase"], a["rm_kf"], a["mp_ref_kf"])
    assert status == c.out["status"]
    same(rows, {k: c.out[k] for k in MC.ROW_KEYS}, name)


@pytest.mark.parametrize("form", [L.frame_sets, L.frame_vec], ids=["sets", "vec"])
@pytest.mark.parametrize("name", list(MC.LOCAL))
def test_local_map_case(name, form):
    c = MC.LOCAL[name]
    fm, lists = L.update_local_map(c.m, np.array([c.args["feat_mp"]], np.int32), MC.local_lists(c), form)
    want_fm, want = MC.local_arrays(c)
    assert fm.dtype == want_fm.dtype and np.array_equal(fm, want_fm), name
    same(lists, want, name)


def refresh(c, batched):
    out = MC.sentinel(len(c.ba["obs_ptr"]) - 1)
    if batched:
        MP.update_map_points_ref(c.m, c.ba, out, c.args["what"])
    else:
        for p in range(len(out["desc"])):
            MP.refresh_point(c.m, c.ba, p, out, c.args["what"])
    return out


@pytest.mark.parametrize("batched", [False, True], ids=["refresh_point", "update_map_points_ref"])
@pytest.mark.parametrize("name", list(MC.POINTS))
def test_points_case(name, batched):
    c = MC.POINTS[name]
    same(refresh(c, batched), MC.points_arrays(c), name)


@pytest.mark.parametrize("batched", [False, True], ids=["refresh_point", "update_map_points_ref"])
@pytest.mark.parametrize("name", list(MC.DESC_SETS) + [None])
def test_descriptor_set(name, batched):
    c = MC.desc_case(name)
    same(refresh(c, batched), MC.points_arrays(c), name)


def row_medians(name):
    d = np.array([MC.segment(*s) for s in MC.DESC_SETS[name][0]])
    D = MP.hamming(d[:, None, :], d[None, :, :])
    return np.sort(D, axis=1)[:, (len(d) - 1) // 2]


@pytest.mark.parametrize("name", list(MC.DESC_SETS))
def test_descriptor_set_conditions(name):
    """from the restatement alone: the row medians that occur are the ones the set was built for; every row in front of the winner has
    a larger median (one computed too small changes the chosen descriptor); the tight sets' winner is one below the front rows"""
    segs, winner, medians = MC.DESC_SETS[name]
    med = row_medians(name)
    assert sorted(set(med.tolist())) == medians, (name, sorted(set(med.tolist())))
    w = MP.distinctive_index(np.array([MC.segment(*s) for s in segs]))
    assert segs[w] == winner and segs.index(winner) == w
    assert name == "tie_first_of_three" or (w > 0 and (med[:w] > med[w]).all()), name
    if name.startswith("n") and name != "n3_far_apart" or (name.startswith("edge_") and int(name.split("_")[1]) <= 160):
        assert med[0] == med[w] + 1  # the front rows sit exactly one above the winner


def test_descriptor_sets_cover_what_the_random_maps_do_not():
    meds = {n: row_medians(n) for n in MC.DESC_SETS}
    assert row_medians("n3_far_apart").min() >= 160
    m = row_medians("tie_first_of_three")
    assert m[0] == m[2] == m.min() and MC.DESC_SETS["tie_first_of_three"][1] == MC.DESC_SETS["tie_first_of_three"][0][0]
    d = np.array([MC.segment(*s) for s in MC.DESC_SETS["distance_256"][0]])
    assert MP.hamming(d[0], d[1]) == 256
    general = set()  # the medians of the sets on the general path (more than 32 observations)
    for n, med in meds.items():
        if len(med) > 32:
            general |= set(med.tolist())
    for edge in range(16, 257, 16):  # both sides of every bin edge of the first radix pass
        assert {edge - 1, edge} <= general, edge
    assert {0, 256} <= general
    assert {len(MC.DESC_SETS[n][0]) for n in MC.DESC_SETS} >= {3, 32, 33, 64, 65, 128, 129}
    assert len(MC.POINTS["n3_n4"].out["desc"]) == 2  # N = 3 and N = 4 by hand, among the moved cases


# ---- the decisions

def declared(c, key):
    return repr(np.asarray(c.out[key]).tolist() if not isinstance(c.out[key], list) else c.out[key])


@pytest.mark.parametrize("entry,what,below,above,outputs,inputs", MC.DECISIONS, ids=[d[1] for d in MC.DECISIONS])
def test_pair_differs_where_stated(entry, what, below, above, outputs, inputs):
    a, b = MC.TABLES[entry][below], MC.TABLES[entry][above]
    assert sorted(a.out) == sorted(b.out)
    differ = tuple(k for k in a.out if declared(a, k) != declared(b, k))
    assert sorted(differ) == sorted(outputs), (what, differ)
    ia, ib = a.inputs(), b.inputs()
    assert sorted(ia) == sorted(ib)
    moved = tuple(k for k in ia if ia[k].shape != ib[k].shape or not np.array_equal(ia[k], ib[k]))
    assert sorted(moved) == sorted(inputs), (what, moved)


def test_every_decision_is_in_the_table():
    """the bullets of the issue, by entry point; the moved cases (local map, the point refresh, kf_first, depth, octave) are cases without a pair"""
    n = {e: sum(1 for d in MC.DECISIONS if d[0] == e) for e in ("conn", "window", "cull", "remove")}
    assert n == dict(conn=10, window=14, cull=8, remove=4), n
    for entry, _, below, above, _, _ in MC.DECISIONS:
        assert below in MC.TABLES[entry] and above in MC.TABLES[entry]
    used = {(d[0], x) for d in MC.DECISIONS for x in d[2:4]}
    alone = {"cull": {"depth_threshold", "octave_plus_one", "kf_first"}, "remove": {"w4_dies_w5_survives", "kf_first_refused"}}
    for entry in ("conn", "window", "cull", "remove"):
        assert {n for n in MC.TABLES[entry] if (entry, n) not in used} == alone.get(entry, set()), entry


# ---- the structural cases

@pytest.mark.parametrize("name", list(MC.STRUCT))
def test_structural_case(name):
    """the selected count sits where the case says (1 023, 1 024 = RANK_LDS, 1 025); both forms agree; the covisible list is the rows
    ascending with every weight 15; the fixed key-frames are NOT in row order"""
    K, NKF, npts, shuffled = MC.STRUCT[name]
    s = MC.struct_case(name)
    conn, win = s["conn"], s["win"]
    v = R.connections_vec(s["m"], 0)
    assert all(np.array_equal(conn[k], v[k]) for k in ("kf_count", "conn_kf", "conn_w"))
    wv = R.window_vec(s["m"], s["ba"], 0)
    assert all(np.array_equal(win[k], wv[k]) for k in R.WINDOW_ARRAYS) and (win["P"], win["F"], win["L"], win["nobs"]) == (wv["P"], wv["F"], wv["L"], wv["nobs"])
    want = int(name.split("_")[1])
    if not shuffled:
        assert len(conn["conn_kf"]) == K == want and conn["conn_kf"].tolist() == list(range(1, K + 1)) and (conn["conn_w"] == 15).all()
        assert (win["P"], win["F"], win["L"], win["nobs"]) == (K + 1, 0, 15, 15 * (K + 1))
    else:
        assert conn["conn_kf"].tolist() == [1] and conn["conn_w"].tolist() == [14]
        assert (win["P"], win["F"], win["L"], win["nobs"]) == (2, K - 1, 14, 14 * (K + 1)) and win["F"] == want
        fixed = win["win_kf"][2:]
        assert sorted(fixed.tolist()) == list(range(2, K + 1)) and (np.diff(fixed) < 0).sum() > want // 4
    assert (NKF <= 4096) == ("global" not in name)
