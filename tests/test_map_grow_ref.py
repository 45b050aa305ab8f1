"""The checker of tests/test_gpu_map_grow.py checked on the CPU: the hand-built scenes of tests/map_grow_scenes.py give their DECLARED
outputs on the model of tests/map_grow_ref.py, every edit leaves a consistent map, gl_map_add's lists say what processNewKeyFrame
does, and each random scene the GPU tests use exercises every branch (a condition on the inputs: the seeds are chosen for it)."""
import numpy as np
import pytest

from tests import map_edit_scenes as ES
from tests import map_grow_ref as G
from tests import map_grow_scenes as GS


def same_as_declared(rows, d, n_points, what):
    want = GS.declared_rows(d, n_points)
    if "kf_valid" in d:
        want["kf_valid"] = np.array(d["kf_valid"], np.uint8)
    for k, v in want.items():
        assert np.array_equal(rows[k], v) and rows[k].dtype == v.dtype, (what, k, rows[k].tolist(), v.tolist())
    assert rows["obs_new_pos"].tolist() == d["new_pos"], (what, rows["obs_new_pos"].tolist())


@pytest.mark.parametrize("name", list(GS.FUSE))
def test_fuse_scenes_give_their_declared_outputs(name):
    sc = GS.hand_scene(GS.FUSE, name)
    M = G.Model(sc["m"], sc["ba"])
    M.check_each = True  # (consistent after EVERY candidate, not only at the end)
    rows, result = G.map_fuse(sc["m"], sc["ba"], 0, sc["cand"], sc["best"], model=M)
    d = sc["out"]
    same_as_declared(rows, d, len(sc["points"]), name)
    assert result == d["result"], (name, result)
    assert list(zip(rows["repl_src"].tolist(), rows["repl_tgt"].tolist())) == d["repl"], name
    M.check_consistent()


def test_fuse_scenes_stand_on_both_sides_of_every_decision():
    """what the names say, from the model's own event counter"""
    ev = {}
    for name in GS.FUSE:
        sc = GS.hand_scene(GS.FUSE, name)
        M = G.Model(sc["m"], sc["ba"])
        G.map_fuse(sc["m"], sc["ba"], 0, sc["cand"], sc["best"], model=M)
        ev[name] = M.events
    assert ev["slot_empty"]["attach"] == 1 and not ev["slot_held_by_an_invalid_point"]
    assert ev["q_heavier"]["cand_into_q"] == 1 and ev["q_lighter"]["q_into_cand"] == 1 and ev["q_lighter"]["tie"] == 0 and ev["tie"]["tie"] == 1
    assert ev["weights_all_stereo"]["cand_into_q"] == 1 and ev["weights_q_mono"]["q_into_cand"] == 1
    assert ev["two_candidates_onto_one_empty_slot"]["attach"] == 1 and ev["two_candidates_onto_one_empty_slot"]["cand_into_q"] == 1
    assert ev["tgt_already_observes"]["nulled"] == 1 and ev["tgt_already_observes"]["chain"] == 0
    assert ev["chain_gained_entry_decides"]["chain"] == 1 and ev["chain_a_into_b_into_c"]["nulled"] == 1
    assert ev["duplicate_after_attach"]["dup_after_attach"] == 1 and ev["duplicate_after_replaced"]["dup_after_replaced"] == 1


def test_two_candidates_verdict_needs_the_attach_counted():
    """the second candidate's verdict flips when the first attach is taken out of the count: the scene tests what it says"""
    sc = GS.hand_scene(GS.FUSE, "two_candidates_onto_one_empty_slot")
    M = G.Model(sc["m"], sc["ba"])
    assert M.points[0].num_obs == 2 and M.points[1].num_obs == 3  # 2 + 2 > 3 > 2


INCONSISTENT_BY_CONSTRUCTION = ("duplicate_triple", "two_triples_onto_one_slot", "two_triples_onto_one_slot_reversed", "walk", "walk_after_triples")  # (ADD scenes whose kf_mp names points that do not observe the slot: that is what they test)


def run_add(sc, check_each=False, **caps):
    n_new = sc.get("new_mp", 0)
    new_mp = GS.new_points(n_new) if n_new else None
    M = G.Model(sc["m"], sc["ba"], sc["mp_ref_kf"])
    M.check_each = check_each
    rows, result = G.map_add(sc["m"], sc["ba"], sc["mp_ref_kf"], new_mp, sc.get("new_kf", ()), sc.get("attach", ()), sc.get("walk", ()), model=M, **caps)
    return rows, result, M, new_mp


@pytest.mark.parametrize("name", list(GS.ADD))
def test_add_scenes_give_their_declared_outputs(name):
    sc = GS.hand_scene(GS.ADD, name)
    rows, result, M, new_mp = run_add(sc, check_each=name not in INCONSISTENT_BY_CONSTRUCTION)  # (consistent after EVERY triple and walk)
    d = sc["out"]
    same_as_declared(rows, d, len(sc["points"]) + sc.get("new_mp", 0), name)
    assert result == d["result"] and rows["already_mp"].tolist() == d["already"], (name, result, rows["already_mp"])
    if new_mp is not None:
        assert np.array_equal(rows["mp_ref_kf"][len(sc["points"]):], new_mp["ref_kf"]) and np.array_equal(rows["new_pos"], new_mp["pos"])
    assert np.array_equal(rows["mp_ref_kf"][:len(sc["points"])], sc["mp_ref_kf"])
    if name not in INCONSISTENT_BY_CONSTRUCTION:
        M.check_consistent()


def test_capacities_exactly_enough_and_one_short():
    sc = GS.hand_scene(GS.ADD, "triples_onto_a_new_point")
    want, result, _, _ = run_add(sc)
    for caps, bits in ((dict(NMPcap=2, OBScap=5), 0), (dict(NMPcap=1, OBScap=5), G.MP_TRUNCATED), (dict(NMPcap=2, OBScap=4), G.OBS_TRUNCATED),
                       (dict(NMPcap=1, OBScap=4), G.MP_TRUNCATED | G.OBS_TRUNCATED)):
        rows, res, _, _ = run_add(sc, **caps)
        assert res == result[:5] + [bits]
        if bits:
            assert all(np.array_equal(rows[k], sc["m"][k]) for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf"))
        else:
            assert all(np.array_equal(rows[k], want[k]) for k in want)
    sc = GS.hand_scene(GS.FUSE, "two_candidates_onto_one_empty_slot")
    NOBS = len(sc["m"]["obs_kf"])
    rows, res = G.map_fuse(sc["m"], sc["ba"], 0, sc["cand"], sc["best"], OBScap=NOBS + 2)
    assert res == sc["out"]["result"]
    rows, res = G.map_fuse(sc["m"], sc["ba"], 0, sc["cand"], sc["best"], OBScap=NOBS + 1)
    assert res == [NOBS + 2, 0, 0, 0, G.OBS_TRUNCATED] and np.array_equal(rows["kf_mp"], sc["m"]["kf_mp"])


@pytest.mark.parametrize("name,seed", GS.RANDOM_ADD)
def test_map_add_with_the_hosts_triples_equals_process_new_key_frame(name, seed):
    """the walk of a key-frame = the triples a host would form for it: (kf_mp[kf][i], kf, i) for every slot whose point is valid and does
    not observe the key-frame yet - the same map either way, and both equal process_new_key_frame called on the model directly"""
    m, ba, ref, lists = GS.add_lists(ES.scene(name, name in ES.CLAMP), seed)
    kf = int(lists["new_kf"][0])
    by_walk, res_w = G.map_add(m, ba, ref, new_kf=[kf], walk_kf=[kf])
    M = G.Model(m, ba, ref)
    tri, seen = [], set()
    for i, p in enumerate(m["kf_mp"][kf]):
        if 0 <= p < len(M.points) and not M.points[p].not_valid and kf not in M.points[p].observations and p not in seen:
            tri.append((int(p), kf, i))
            seen.add(int(p))
    assert len(tri) >= 2
    by_tri, res_t = G.map_add(m, ba, ref, new_kf=[kf], attach=tri)
    direct = G.Model(m, ba, ref)
    direct.kfs[kf].not_valid = False
    cands, n = direct.process_new_key_frame(direct.kfs[kf])
    rows = direct.to_rows()
    for k in rows:
        assert np.array_equal(by_walk[k], rows[k]) and np.array_equal(by_tri[k], rows[k]), k
    assert res_w[:3] == res_t[:3] == [len(M.points), len(rows["obs_kf"]), n] and by_walk["already_mp"].tolist() == cands and len(cands) > 0
    direct.check_consistent()


def every_fuse_branch(ev, what):
    print(what, dict(ev))
    assert ev["attach"] >= 1 and ev["cand_into_q"] >= 1 and ev["q_into_cand"] >= 1 and ev["nulled"] >= 1 and ev["chain"] >= 1, what
    assert ev["dup_after_attach"] + ev["dup_after_replaced"] >= 1, what


def test_the_fuse_list_on_the_grown_map_exercises_every_branch():
    """the list tests/test_gpu_map_grow.py makes on the map a device add leaves (GS.grown_lists): the same condition on the inputs"""
    g = GS.grown_lists()
    M = G.Model(g["m1"], g["ba1"])
    rows, result = G.map_fuse(g["m1"], g["ba1"], g["kf"], g["cand"], g["best"], model=M)
    every_fuse_branch(M.events, (GS.GROWN, result))
    assert g["res1"][2] > 20 and result[3] >= 3


@pytest.mark.parametrize("name,seed", GS.RANDOM_FUSE + (GS.BIG_FUSE,))
def test_random_fuse_scenes_exercise_every_branch(name, seed):
    sc = ES.scene(name, name in ES.CLAMP)
    kf, cand, best = GS.fuse_lists(sc, seed)
    M = G.Model(sc["m"], sc["ba"])
    M.check_each = name != "euroc"  # (after every candidate; the big scene once at the end: a check walks 180 000 points)
    rows, result = G.map_fuse(sc["m"], sc["ba"], kf, cand, best, model=M)
    every_fuse_branch(M.events, (name, seed, result))
    M.check_consistent()
    assert rows["obs_ptr"][-1] == len(rows["obs_kf"]) == result[0]
    moved = rows["obs_new_pos"][rows["obs_new_pos"] >= 0]
    assert len(np.unique(moved)) == len(moved)


@pytest.mark.parametrize("name,seed", GS.RANDOM_ADD + (GS.BIG_ADD,))
def test_random_add_scenes_exercise_every_branch(name, seed):
    m, ba, ref, lists = GS.add_lists(ES.scene(name, name in ES.CLAMP), seed)
    M = G.Model(m, ba, ref)
    rows, result = G.map_add(m, ba, ref, lists["new_mp"], lists["new_kf"], lists["attach"], lists["walk_kf"], model=M)
    print(name, seed, dict(M.events), result)
    assert M.events["attach"] >= 2 * len(lists["new_mp"]["pos"]) and M.events["dup_triple"] >= 1 and M.events["skipped"] >= 6
    assert result[2] > M.events["attach"] and result[4] >= 1  # the walk attached some and found others observing
    att = lists["attach"]
    slots = att[:, 1].astype(np.int64) * 1000 + att[:, 2]
    assert len(np.unique(slots)) < len(slots)  # several triples onto one slot
    assert (rows["obs_new_pos"] >= 0).all() and rows["kf_valid"][lists["new_kf"][0]] == 1
