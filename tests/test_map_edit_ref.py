"""The three facts gl_cull_keyframes / gl_map_remove rest on (gmmloc_hip.h), held by the sequential object model of
tests/map_edit_ref.py alone, hand-built cases (the maps and declared outputs of tests/map_cases.py) with their expected arrays written out, and the conditions the scenes of
tests/map_edit_scenes.py must meet so that tests/test_gpu_map_edit.py cannot pass vacuously.  No GPU."""
import numpy as np
import pytest

from tests import ba_window_scenes as S
from tests import map_cases as MC
from tests import map_edit_ref as E
from tests import map_edit_scenes as ES

INF = 2 ** 31 - 1
ROW_KEYS = ("mp_valid", "kf_valid", "obs_ptr", "obs_kf", "obs_feat", "obs_new_pos", "dead_mp", "mp_ref_kf")


# ---- the closed form of "the points, then the observations, then the key-frames in list order", vectorised, written apart from the model

def closed_form(m, ba, rm_mp, erase, rm_kf, mp_ref_kf):
    """-> the rows of Model.to_rows, on a CONSISTENT map"""
    NMP, NKF, NFK, NOBS = E._sizes(m)
    mpv, kfv = m["mp_valid"] != 0, m["kf_valid"] != 0
    ptr, okf, of = m["obs_ptr"].astype(np.int64), m["obs_kf"].astype(np.int64), ba["obs_feat"].astype(np.int64)
    pt = np.repeat(np.arange(NMP), np.diff(ptr))
    rank = np.full(NKF, INF, np.int64)
    for i, k in enumerate(rm_kf):
        if 0 <= k < NKF and kfv[k] and k != ba["kf_first"]:
            rank[k] = min(rank[k], i)
    er = np.zeros(NOBS, bool)
    er[[o for o in erase if 0 <= o < NOBS]] = True
    pf = np.zeros(NMP, bool)
    pf[[p for p in rm_mp if 0 <= p < NMP]] = True
    pf &= mpv
    wgt = np.where(ba["kf_uvr"][okf, of, 2] >= 0, 2, 1)
    rk = rank[okf]
    gone = er | (rk < INF)
    w_keep = np.bincount(pt, wgt * ~gone, NMP)
    dead = mpv & (pf | ((np.bincount(pt, gone, NMP) > 0) & (w_keep <= 2)))
    w1 = np.bincount(pt, wgt * ~er, NMP)
    t = np.full(NMP, INF, np.int64)
    t[dead & (pf | ((np.bincount(pt, er, NMP) > 0) & (w1 <= 2)))] = -1
    for p in np.nonzero(dead & (t == INF))[0]:  # the removed observers in ascending rank: the first that leaves w <= 2
        e = np.arange(ptr[p], ptr[p + 1])
        e = e[~er[e] & (rk[e] < INF)]
        w = w1[p]
        for o in e[np.argsort(rk[e])]:
            w -= wgt[o]
            if w <= 2:
                t[p] = rk[o]
                break
    lost = mpv[pt] & (dead[pt] | gone)
    clear = mpv[pt] & (er | (dead[pt] & ((rk == INF) | (t[pt] < rk))))
    kf_mp = m["kf_mp"].copy()
    sel = clear & (kf_mp[okf, of] == pt)
    kf_mp[okf[sel], of[sel]] = -1
    keep = ~lost
    nptr = np.zeros(NMP + 1, np.int64)
    nptr[1:] = np.cumsum(np.bincount(pt, keep, NMP))
    new_pos = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    ref = mp_ref_kf.copy()
    ref_lost = np.bincount(pt, lost & (okf == mp_ref_kf[pt]), NMP) > 0
    alive = mpv & ~dead & ref_lost & (np.diff(nptr) > 0)
    ref[alive] = okf[keep][nptr[:-1][alive]]
    kf_valid = m["kf_valid"].copy()
    kf_valid[rank < INF] = 0
    return dict(mp_valid=(mpv & ~dead).astype(np.uint8), kf_valid=kf_valid, kf_mp=kf_mp, obs_ptr=nptr.astype(np.int32), obs_kf=okf[keep].astype(np.int32),
                obs_feat=of[keep].astype(np.int32), obs_new_pos=new_pos, dead_mp=np.nonzero(dead)[0].astype(np.int32), mp_ref_kf=ref), t


def same_rows(a, b, what, mask_rows=None):
    for k in ROW_KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)
    x, y = a["kf_mp"].copy(), b["kf_mp"].copy()
    if mask_rows is not None:
        x[mask_rows], y[mask_rows] = -9, -9
    assert np.array_equal(x, y), (what, "kf_mp")


def run_ops(sc, ops):
    M = E.Model(sc["m"], sc["ba"], sc["mp_ref_kf"])
    for kind, x in ops:
        if kind == "mp":
            M.remove_map_point(M.points[x])
        elif kind == "obs":
            M.ba_erase([x])
        else:
            M.remove_key_frame(M.kfs[x])
    return M.to_rows()


@pytest.mark.parametrize("name", S.SMALL)
def test_fact_1_removals_commute_outside_the_removed_rows(name):
    """the same removals in 24 random orders, the three kinds interleaved: identical rows with the removed key-frames' own rows masked,
    and identical to the closed form"""
    sc = ES.scene(name)
    rm_mp, erase, rm_kf = ES.removals(sc, 3)
    ops = [("mp", int(p)) for p in rm_mp] + [("obs", int(o)) for o in erase] + [("kf", int(k)) for k in rm_kf]
    first = run_ops(sc, ops)
    cf, _ = closed_form(sc["m"], sc["ba"], rm_mp, erase, rm_kf, sc["mp_ref_kf"])
    same_rows(first, cf, name + " closed form", rm_kf)
    assert len(first["dead_mp"]) > len(rm_mp) and len(first["obs_kf"]) < len(sc["m"]["obs_kf"])
    rng = np.random.default_rng(5)
    for trial in range(24):
        order = [ops[i] for i in rng.permutation(len(ops))]
        same_rows(run_ops(sc, order), first, (name, trial), rm_kf)


@pytest.mark.parametrize("name", S.SMALL)
def test_fact_2_the_removed_rows_follow_the_list_order(name):
    """in the prescribed order the removed key-frames' rows equal the t(p) < i rule (the closed form, unmasked); on `small` the reversed
    list gives DIFFERENT rows, and the rule follows it"""
    sc = ES.scene(name)
    rm_mp, erase, rm_kf = ES.removals(sc, 3)
    differs = False
    for lst in (rm_kf, rm_kf[::-1].copy()):
        rows, status = E.map_remove(sc["m"], sc["ba"], rm_mp, erase, lst, sc["mp_ref_kf"])
        cf, t = closed_form(sc["m"], sc["ba"], rm_mp, erase, lst, sc["mp_ref_kf"])
        assert status == 0
        same_rows(rows, cf, name)
        if lst is rm_kf:
            fwd = rows
            assert ((t >= 0) & (t < INF)).any() or name != "small"  # points that die at a key-frame's removal
        else:
            differs = not np.array_equal(rows["kf_mp"][rm_kf], fwd["kf_mp"][rm_kf])
            same_rows(rows, fwd, name + " reversed", rm_kf)
    assert differs or name != "small"


@pytest.mark.parametrize("name,clamp", [(n, False) for n in S.SMALL] + [(n, True) for n in ES.CLAMP])
def test_fact_3_the_loop_reads_a_function_of_the_culled_set(name, clamp):
    sc = ES.scene(name, clamp)
    seq = E.Model(sc["m"], sc["ba"]).remove_key_frames(sc["cand"], sc["kf_depth"], sc["th_depth"])
    fc = E.cull_by_state(sc["m"], sc["ba"], sc["cand"], sc["kf_depth"], sc["th_depth"])
    for k in seq:
        assert np.array_equal(seq[k], fc[k]), (name, clamp, k)
    rev = sc["cand"][::-1].copy()
    a, b = E.Model(sc["m"], sc["ba"]).remove_key_frames(rev, sc["kf_depth"], sc["th_depth"]), E.cull_by_state(sc["m"], sc["ba"], rev, sc["kf_depth"], sc["th_depth"])
    for k in a:
        assert np.array_equal(a[k], b[k]), (name, clamp, "reversed", k)


def independent_verdicts(sc):
    return np.array([E.cull_by_state(sc["m"], sc["ba"], [k], sc["kf_depth"], sc["th_depth"])["cull"][0] for k in sc["cand"]], np.uint8)


@pytest.mark.parametrize("name", list(ES.CLAMP))
def test_scene_conditions_clamped(name):
    """at least 3 culled; a verdict in list order differs from the verdict on the unedited map; a point dies by the cascade; a surviving
    point changes mp_ref_kf"""
    sc = ES.scene(name, True)
    M = E.Model(sc["m"], sc["ba"], sc["mp_ref_kf"])
    r = M.remove_key_frames(sc["cand"], sc["kf_depth"], sc["th_depth"])
    rows = M.to_rows()
    alone = independent_verdicts(sc)
    print(name, "culled in list order", int(r["cull"].sum()), "independently", int(alone.sum()), "differ", int((alone != r["cull"]).sum()), "deaths",
          len(rows["dead_mp"]), "ref changes", int(((rows["mp_ref_kf"] != sc["mp_ref_kf"]) & (rows["mp_valid"] != 0)).sum()))
    assert r["cull"].sum() >= 3
    assert (alone != r["cull"]).any()
    assert len(rows["dead_mp"]) >= 1
    assert ((rows["mp_ref_kf"] != sc["mp_ref_kf"]) & (rows["mp_valid"] != 0)).any()
    # the same through gl_map_remove's semantics: the culled rows as rm_kf
    again, status = E.map_remove(sc["m"], sc["ba"], rm_kf=r["cull_rows"], mp_ref_kf=sc["mp_ref_kf"])
    assert status == 0
    same_rows(again, rows, name)


@pytest.mark.parametrize("name", S.SMALL)
def test_scene_conditions_unclamped(name):
    sc = ES.scene(name)
    r = E.cull_by_state(sc["m"], sc["ba"], sc["cand"], sc["kf_depth"], sc["th_depth"])
    part = (r["num_redundant"] > 0) & (r["num_redundant"] < r["num_mps"])
    print(name, "culled", int(r["cull"].sum()), "partly redundant", int(part.sum()), "of", len(sc["cand"]))
    assert part.any()


# ---- hand-built cases: the maps, the lists and the declared outputs are in tests/map_cases.py (REMOVE, CULL), which
# tests/test_gpu_map_cases.py runs on the device as well

def test_a_stereo_point_with_w4_dies_and_one_with_w5_survives():
    # point 0: two stereo observers (w = 4); point 1: two stereo + one mono (w = 5); the observation by key-frame 1 is erased from both
    c = MC.REMOVE["w4_dies_w5_survives"]
    m, ba = c.m, c.ba
    assert c.args["erase"].tolist() == [0, 2] and c.args["mp_ref_kf"].tolist() == [1, 1]
    rows, _ = E.map_remove(m, ba, erase_obs=c.args["erase"], mp_ref_kf=c.args["mp_ref_kf"])
    assert rows["mp_valid"].tolist() == [0, 1] and rows["dead_mp"].tolist() == [0]
    assert rows["obs_ptr"].tolist() == [0, 0, 2] and rows["obs_kf"].tolist() == [2, 3] and rows["obs_feat"].tolist() == [1, 0]
    assert rows["obs_new_pos"].tolist() == [-1, -1, -1, 0, 1]
    assert rows["kf_mp"].tolist() == [[-1, -1], [-1, -1], [-1, 1], [1, -1]]
    assert rows["mp_ref_kf"].tolist() == [1, 2]  # the dead point keeps its entry, the survivor takes its first surviving observer
    cf, _ = closed_form(m, ba, [], [0, 2], [], np.array([1, 1], np.int32))
    same_rows(rows, cf, "w4 / w5")


@pytest.mark.parametrize("name,order,expect", [("three_observers_123", [1, 2, 3], [[-1], [0], [0], [-1]]), ("three_observers_321", [3, 2, 1], [[-1], [-1], [0], [0]])],
                         ids=["order0-expect0", "order1-expect1"])
def test_three_observers_in_both_orders(name, order, expect):
    """a point with the three stereo observers 1, 2, 3 (w = 6), all three removed.  The first removal leaves w = 4, the second w = 2:
    the point dies at step 1.  The key-frame removed first keeps its slot (nothing nulls a removed key-frame's own row), the second
    keeps it too (its own removal kills the point: it no longer observes it), the third still observes the dying point: CLEARED."""
    c = MC.REMOVE[name]
    m, ba = c.m, c.ba
    assert c.args["rm_kf"].tolist() == order and c.out["kf_mp"].tolist() == expect
    rows, _ = E.map_remove(m, ba, rm_kf=order)
    assert rows["mp_valid"].tolist() == [0] and rows["kf_valid"].tolist() == [1, 0, 0, 0] and rows["obs_ptr"].tolist() == [0, 0]
    assert rows["kf_mp"].tolist() == expect
    cf, t = closed_form(m, ba, [], [], order, np.zeros(1, np.int32))
    assert cf["kf_mp"].tolist() == expect and t[0] == 1


def test_the_rank_decides_the_removed_rows():
    """point 0: observers 1, 2 (stereo), 3, 4 (mono), w = 6; point 1: observers 3, 4, 0 (stereo), w = 6; key-frames 1, 2, 3 removed.
    [1, 2, 3]: point 0 goes 6 -> 4 -> 2 and dies at step 1; key-frame 3 (rank 2) still observes it: its slot is cleared.
    [3, 2, 1]: 6 -> 5 -> 3 -> 1, dies at step 2: no removed row is touched.  Point 1 survives with w = 4 either way and key-frame 3
    keeps its slot; the remaining observer 4 of point 0 is cleared either way."""
    ca, cb = MC.REMOVE["rank_123"], MC.REMOVE["rank_321"]
    m, ba = ca.m, ca.ba
    assert all(np.array_equal(ca.m[k], cb.m[k]) for k in ca.m) and ca.args["rm_kf"].tolist() == [1, 2, 3] and cb.args["rm_kf"].tolist() == [3, 2, 1]
    a, _ = E.map_remove(m, ba, rm_kf=[1, 2, 3])
    b, _ = E.map_remove(m, ba, rm_kf=[3, 2, 1])
    assert a["kf_mp"].tolist() == [[1, -1], [0, -1], [0, -1], [-1, 1], [-1, 1]]
    assert b["kf_mp"].tolist() == [[1, -1], [0, -1], [0, -1], [0, 1], [-1, 1]]
    for r in (a, b):
        assert r["mp_valid"].tolist() == [0, 1] and r["obs_ptr"].tolist() == [0, 0, 2] and r["obs_kf"].tolist() == [4, 0]
    for lst, r in (([1, 2, 3], a), ([3, 2, 1], b)):
        cf, t = closed_form(m, ba, [], [], lst, np.zeros(2, np.int32))
        assert np.array_equal(cf["kf_mp"], r["kf_mp"]) and t[0] == (1 if lst[0] == 1 else 2)


def test_kf_first_is_never_culled_and_never_removed():
    c = MC.CULL["kf_first"]
    m, ba, depth = c.m, c.ba, c.args["kf_depth"]
    assert ba["kf_first"] == 0 and c.args["cand"] == [0, 1] and c.args["th_depth"] == 6.0
    for judge in (lambda: E.Model(m, ba).remove_key_frames([0, 1], depth, 6.0), lambda: E.cull_by_state(m, ba, [0, 1], depth, 6.0)):
        r = judge()
        assert r["status"].tolist() == [E.FIRST, E.JUDGED] and r["cull"].tolist() == [0, 1] and r["num_mps"].tolist() == [0, 4]
    rows, status = E.map_remove(m, ba, rm_kf=[0])
    assert status == E.FIRST_REFUSED and rows["kf_valid"].tolist() == [1, 1, 1, 1] and np.array_equal(rows["obs_kf"], m["obs_kf"])


@pytest.mark.parametrize("name,redundant,cull", [("ninety_10_at", 9, 0), ("ninety_10_over", 10, 1)], ids=["9-0", "10-1"])
def test_the_ninety_percent_boundary(name, redundant, cull):
    """ten counted points on key-frame 1; `redundant` of them have three other observers, the rest two: 9 of 10 is not culled
    (9 > 0.9 * 10 is false), 10 of 10 is"""
    c = MC.CULL[name]
    m, ba, depth = c.m, c.ba, c.args["kf_depth"]
    assert (np.diff(m["obs_ptr"]) == 4).sum() == redundant and len(m["mp_valid"]) == 10
    for r in (E.Model(m, ba).remove_key_frames([1], depth, 6.0), E.cull_by_state(m, ba, [1], depth, 6.0)):
        assert r["num_mps"].tolist() == [10] and r["num_redundant"].tolist() == [redundant] and r["cull"].tolist() == [cull]


def test_depth_at_the_threshold_counts_and_above_does_not():
    c = MC.CULL["depth_threshold"]
    m, ba, depth = c.m, c.ba, c.args["kf_depth"]
    assert depth[1].tolist() == [6.0, float(np.nextafter(np.float32(6.0), np.float32(7.0))), -1.0, 0.0]
    for r in (E.Model(m, ba).remove_key_frames([1], depth, 6.0), E.cull_by_state(m, ba, [1], depth, 6.0)):
        assert r["num_mps"].tolist() == [2] and r["num_redundant"].tolist() == [2]


def test_octave_scale_plus_one_counts_and_plus_two_does_not():
    """key-frame 1 sees both points at octave 2; point 0's other observers sit at octave 3 (counted), point 1's at 4 (not)"""
    c = MC.CULL["octave_plus_one"]
    m, ba, depth = c.m, c.ba, c.args["kf_depth"]
    assert ba["kf_oct"].tolist() == [[0, 0], [2, 2], [3, 4], [3, 4], [3, 4]]
    for r in (E.Model(m, ba).remove_key_frames([1], depth, 6.0), E.cull_by_state(m, ba, [1], depth, 6.0)):
        assert r["num_mps"].tolist() == [2] and r["num_redundant"].tolist() == [1] and r["cull"].tolist() == [0]


def test_lists_with_entries_that_change_nothing():
    sc = ES.scene("small")
    rm_mp, erase, rm_kf = ES.removals(sc, 3)
    clean, s0 = E.map_remove(sc["m"], sc["ba"], rm_mp, erase, rm_kf, sc["mp_ref_kf"])
    d_mp, d_er, d_kf = ES.dirty(sc, rm_mp, erase, rm_kf)
    dirty, s1 = E.map_remove(sc["m"], sc["ba"], d_mp, d_er, d_kf, sc["mp_ref_kf"])
    assert (s0, s1) == (0, E.FIRST_REFUSED)
    same_rows(dirty, clean, "dirty lists")
    r = E.Model(sc["m"], sc["ba"]).remove_key_frames(d_kf, sc["kf_depth"], sc["th_depth"])
    assert {E.FIRST, E.BAD_ROW, E.INVALID, E.DUPLICATE, E.JUDGED} == set(r["status"].tolist())
