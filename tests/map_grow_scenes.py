"""The scenes of tests/test_map_grow_ref.py (CPU: the declared outputs, the conditions that keep the GPU tests from passing vacuously)
and tests/test_gpu_map_grow.py (GPU: gl_map_add / gl_map_fuse against tests/map_grow_ref.py).  Test infrastructure; nothing in the
product imports it.

HAND-BUILT: six key-frames of eight features, a handful of points, one scene on each side of every decision, each with its output
DECLARED by hand - `obs` (every point's observations (key-frame, feature) in CSR order), `valid`, `slots` (every kf_mp slot that holds
a point), `result` and the lists.  A feature is stereo (weight 2) unless `mono` names it.  Fuse scenes work on key-frame 0.
RANDOM: the maps of tests/map_edit_scenes.py with deliberately colliding lists, pinned seeds."""
import numpy as np

from gmmloc_amd import api, synth
from tests import map_edit_scenes as ES

NKF, NFK = 6, 8


def build(points, invalid_mp=(), invalid_kf=(), mono=(), extra_slots=None):
    """points: per point its observations [(kf, feat), ...] in CSR order -> (m, ba, mp_ref_kf); kf_mp holds every observation (those of
    the invalid points too) and extra_slots {(kf, feat): mp} on top"""
    NMP = len(points)
    kf_mp = -np.ones((NKF, NFK), np.int32)
    for p, obs in enumerate(points):
        for k, f in obs:
            kf_mp[k, f] = p
    for (k, f), p in (extra_slots or {}).items():
        kf_mp[k, f] = p
    ptr = np.zeros(NMP + 1, np.int32)
    ptr[1:] = np.cumsum([len(o) for o in points])
    mpv, kfv = np.ones(NMP, np.uint8), np.ones(NKF, np.uint8)
    mpv[list(invalid_mp)] = 0
    kfv[list(invalid_kf)] = 0
    m = dict(mp_valid=mpv, kf_valid=kfv, kf_mp=kf_mp, obs_ptr=ptr, obs_kf=np.array([k for o in points for k, _ in o], np.int32),
             mp_pos=np.arange(NMP * 3, dtype=np.float64).reshape(NMP, 3))
    uvr = np.ones((NKF, NFK, 3))
    for k, f in mono:
        uvr[k, f, 2] = -1.0
    ba = dict(kf_uvr=uvr, kf_oct=np.zeros((NKF, NFK), np.int32), obs_feat=np.array([f for o in points for _, f in o], np.int32),
              mp_assoc=np.arange(NMP, dtype=np.int32) + 100, kf_first=-1)
    return m, ba, np.array([o[0][0] if o else -1 for o in points], np.int32)


def declared_rows(d, n_points):
    """the arrays a declared output stands for: mp_valid, kf_mp, obs_ptr, obs_kf, obs_feat"""
    kf_mp = -np.ones((NKF, NFK), np.int32)
    for (k, f), p in d["slots"].items():
        kf_mp[k, f] = p
    ptr = np.zeros(n_points + 1, np.int32)
    ptr[1:] = np.cumsum([len(o) for o in d["obs"]])
    return dict(mp_valid=np.array(d["valid"], np.uint8), kf_mp=kf_mp, obs_ptr=ptr, obs_kf=np.array([k for o in d["obs"] for k, _ in o], np.int32),
                obs_feat=np.array([f for o in d["obs"] for _, f in o], np.int32))


A_LIGHT = [(3, 0)]                    # weight 2
Q_HEAVY = [(0, 3), (1, 1), (2, 1)]    # weight 6, holds slot (0, 3)

# name -> dict(points, [invalid_mp, mono, extra_slots], cand, best, out = dict(obs, valid, slots, result, repl, new_pos))
FUSE = {
    "slot_empty": dict(
        points=[[(1, 0), (2, 0)]], cand=[0], best=[3],
        out=dict(obs=[[(1, 0), (2, 0), (0, 3)]], valid=[1], slots={(1, 0): 0, (2, 0): 0, (0, 3): 0}, result=[3, 1, 1, 0, 0], repl=[], new_pos=[0, 1])),
    "slot_held_by_an_invalid_point": dict(
        points=[[(1, 0), (2, 0)], [(0, 3), (1, 1)]], invalid_mp=[1], cand=[0], best=[3],
        out=dict(obs=[[(1, 0), (2, 0)], [(0, 3), (1, 1)]], valid=[1, 0], slots={(1, 0): 0, (2, 0): 0, (0, 3): 1, (1, 1): 1}, result=[4, 1, 0, 0, 0],
                 repl=[], new_pos=[0, 1, 2, 3])),
    "q_heavier": dict(  # w(q) = 6 > w(cand) = 2: the candidate goes into q, its entry moves behind q's
        points=[A_LIGHT, Q_HEAVY], cand=[0], best=[3],
        out=dict(obs=[[], Q_HEAVY + [(3, 0)]], valid=[0, 1], slots={(0, 3): 1, (1, 1): 1, (2, 1): 1, (3, 0): 1}, result=[4, 1, 0, 1, 0], repl=[(0, 1)],
                 new_pos=[3, 0, 1, 2])),
    "tie": dict(  # 2 == 2: q goes into the candidate
        points=[[(3, 0)], [(0, 3)]], cand=[0], best=[3],
        out=dict(obs=[[(3, 0), (0, 3)], []], valid=[1, 0], slots={(3, 0): 0, (0, 3): 0}, result=[2, 1, 0, 1, 0], repl=[(1, 0)], new_pos=[0, 1])),
    "q_lighter": dict(  # w(q) = 2 < w(cand) = 4
        points=[[(3, 0), (4, 0)], [(0, 3)]], cand=[0], best=[3],
        out=dict(obs=[[(3, 0), (4, 0), (0, 3)], []], valid=[1, 0], slots={(3, 0): 0, (4, 0): 0, (0, 3): 0}, result=[3, 1, 0, 1, 0], repl=[(1, 0)],
                 new_pos=[0, 1, 2])),
    "weights_all_stereo": dict(  # two entries against three, all stereo: 4 < 6, the candidate goes into q ...
        points=[[(3, 0), (4, 0)], Q_HEAVY], cand=[0], best=[3],
        out=dict(obs=[[], Q_HEAVY + [(3, 0), (4, 0)]], valid=[0, 1], slots={(0, 3): 1, (1, 1): 1, (2, 1): 1, (3, 0): 1, (4, 0): 1}, result=[5, 1, 0, 1, 0],
                 repl=[(0, 1)], new_pos=[3, 4, 0, 1, 2])),
    "weights_q_mono": dict(  # ... the same entries with q's three monocular: 4 > 3, q goes into the candidate
        points=[[(3, 0), (4, 0)], Q_HEAVY], mono=Q_HEAVY, cand=[0], best=[3],
        out=dict(obs=[[(3, 0), (4, 0)] + Q_HEAVY, []], valid=[1, 0], slots={(0, 3): 0, (1, 1): 0, (2, 1): 0, (3, 0): 0, (4, 0): 0}, result=[5, 1, 0, 1, 0],
                 repl=[(1, 0)], new_pos=[0, 1, 2, 3, 4])),
    "two_candidates_onto_one_empty_slot": dict(  # point 0 attaches (2 -> 4); point 1 (3) then meets it: 4 > 3 only with the attach counted
        points=[[(1, 0)], [(2, 0), (3, 0)]], mono=[(3, 0)], cand=[0, 1], best=[3, 3],
        out=dict(obs=[[(1, 0), (0, 3), (2, 0), (3, 0)], []], valid=[1, 0], slots={(1, 0): 0, (0, 3): 0, (2, 0): 0, (3, 0): 0}, result=[4, 2, 1, 1, 0],
                 repl=[(1, 0)], new_pos=[0, 2, 3])),
    "tgt_already_observes": dict(  # the candidate's (1, 0): q observes key-frame 1 - the slot is nulled, the entry gone
        points=[[(1, 0), (3, 0)], Q_HEAVY], cand=[0], best=[3],
        out=dict(obs=[[], Q_HEAVY + [(3, 0)]], valid=[0, 1], slots={(0, 3): 1, (1, 1): 1, (2, 1): 1, (3, 0): 1}, result=[4, 1, 0, 1, 0], repl=[(0, 1)],
                 new_pos=[-1, 3, 0, 1, 2])),
    "chain_gained_entry_decides": dict(  # A = 0 goes into B = 1, which gains (4, 0); C = 2 meets B: only that gained entry nulls C's (4, 1)
        points=[[(4, 0)], [(0, 3), (1, 1)], [(4, 1), (5, 0)]], cand=[0, 2], best=[3, 3],
        out=dict(obs=[[], [(0, 3), (1, 1), (4, 0), (5, 0)], []], valid=[0, 1, 0], slots={(0, 3): 1, (1, 1): 1, (4, 0): 1, (5, 0): 1}, result=[4, 2, 0, 2, 0],
                 repl=[(0, 1), (2, 1)], new_pos=[2, 0, 1, -1, 3])),
    "chain_a_into_b_into_c": dict(  # A into B, then B (6) into C (8): A's entry is walked as B's and nulled, C observes key-frame 4
        points=[[(4, 0)], [(0, 3), (1, 1)], [(2, 0), (3, 0), (4, 1), (5, 0)]], cand=[0, 2], best=[3, 3],
        out=dict(obs=[[], [], [(2, 0), (3, 0), (4, 1), (5, 0), (0, 3), (1, 1)]], valid=[0, 0, 1],
                 slots={(2, 0): 2, (3, 0): 2, (4, 1): 2, (5, 0): 2, (0, 3): 2, (1, 1): 2}, result=[6, 2, 0, 2, 0], repl=[(0, 1), (1, 2)],
                 new_pos=[-1, 4, 5, 0, 1, 2, 3])),
    "duplicate_after_attach": dict(  # the second time it observes key-frame 0 by its own attach
        points=[[(1, 0)]], cand=[0, 0], best=[3, 4],
        out=dict(obs=[[(1, 0), (0, 3)]], valid=[1], slots={(1, 0): 0, (0, 3): 0}, result=[2, 1, 1, 0, 0], repl=[], new_pos=[0])),
    "duplicate_after_replaced": dict(  # the second time it is invalid
        points=[A_LIGHT, Q_HEAVY], cand=[0, 0], best=[3, 4],
        out=dict(obs=[[], Q_HEAVY + [(3, 0)]], valid=[0, 1], slots={(0, 3): 1, (1, 1): 1, (2, 1): 1, (3, 0): 1}, result=[4, 1, 0, 1, 0], repl=[(0, 1)],
                 new_pos=[3, 0, 1, 2])),
    "candidate_invalid_or_observing": dict(  # point 2 is invalid, point 0 observes key-frame 0 on entry
        points=[[(0, 1), (1, 0)], [(0, 3), (2, 0)], [(3, 0)]], invalid_mp=[2], cand=[2, 0], best=[3, 3],
        out=dict(obs=[[(0, 1), (1, 0)], [(0, 3), (2, 0)], [(3, 0)]], valid=[1, 1, 0], slots={(0, 1): 0, (1, 0): 0, (0, 3): 1, (2, 0): 1, (3, 0): 2},
                 result=[5, 0, 0, 0, 0], repl=[], new_pos=[0, 1, 2, 3, 4])),
    "rows_out_of_range": dict(  # candidate rows and features outside the tables: nothing is a match
        points=[A_LIGHT, Q_HEAVY], cand=[-1, 2, 0, 0, 2 ** 31 - 1], best=[3, 3, -1, NFK, 3],
        out=dict(obs=[A_LIGHT, Q_HEAVY], valid=[1, 1], slots={(3, 0): 0, (0, 3): 1, (1, 1): 1, (2, 1): 1}, result=[4, 0, 0, 0, 0], repl=[],
                 new_pos=[0, 1, 2, 3])),
}

# name -> dict(points, [...], new_mp (count), new_kf, attach, walk, out = dict(obs, valid, kf_valid, slots, result, already, new_pos))
ADD = {
    "duplicate_triple": dict(  # the second triple of (point 0, key-frame 2): the point side does nothing, the key-frame side writes its slot
        points=[[(1, 0)]], attach=[(0, 2, 3), (0, 2, 4)],
        out=dict(obs=[[(1, 0), (2, 3)]], valid=[1], slots={(1, 0): 0, (2, 3): 0, (2, 4): 0}, result=[1, 2, 1, 0, 0, 0], already=[], new_pos=[0])),
    "two_triples_onto_one_slot": dict(  # the LAST one owns the slot ...
        points=[[(1, 0)], [(1, 1)]], attach=[(0, 2, 3), (1, 2, 3)],
        out=dict(obs=[[(1, 0), (2, 3)], [(1, 1), (2, 3)]], valid=[1, 1], slots={(1, 0): 0, (1, 1): 1, (2, 3): 1}, result=[2, 4, 2, 0, 0, 0], already=[],
                 new_pos=[0, 2])),
    "two_triples_onto_one_slot_reversed": dict(  # ... in either order
        points=[[(1, 0)], [(1, 1)]], attach=[(1, 2, 3), (0, 2, 3)],
        out=dict(obs=[[(1, 0), (2, 3)], [(1, 1), (2, 3)]], valid=[1, 1], slots={(1, 0): 0, (1, 1): 1, (2, 3): 0}, result=[2, 4, 2, 0, 0, 0], already=[],
                 new_pos=[0, 2])),
    "triples_onto_a_new_point": dict(  # a new row with two observations, as createMapPoints makes it; the old point's triple keeps list order
        points=[[(1, 0)]], new_mp=1, attach=[(1, 2, 5), (0, 3, 1), (1, 1, 5), (0, 2, 2)],
        out=dict(obs=[[(1, 0), (3, 1), (2, 2)], [(2, 5), (1, 5)]], valid=[1, 1], slots={(1, 0): 0, (3, 1): 0, (2, 2): 0, (2, 5): 1, (1, 5): 1},
                 result=[2, 5, 4, 0, 0, 0], already=[], new_pos=[0])),
    "walk": dict(  # key-frame 2's slots: 0 holds point 0 (observes it: already), 1 and 3 point 1 (gains (2, 1), then already), 2 an invalid point
        points=[[(2, 0), (1, 0)], [(1, 1)], [(1, 2)]], invalid_mp=[2], extra_slots={(2, 1): 1, (2, 2): 2, (2, 3): 1}, walk=[2, 2, -1, NKF],
        out=dict(obs=[[(2, 0), (1, 0)], [(1, 1), (2, 1)], [(1, 2)]], valid=[1, 1, 0],
                 slots={(2, 0): 0, (1, 0): 0, (1, 1): 1, (1, 2): 2, (2, 1): 1, (2, 2): 2, (2, 3): 1}, result=[3, 5, 1, 0, 2, 0], already=[0, 1],
                 new_pos=[0, 1, 2, 4])),
    "walk_after_triples": dict(  # the triple takes slot (2, 1) from point 1 before the walk reads it; point 0 then observes by its triple
        points=[[(1, 0)], [(1, 1)]], extra_slots={(2, 1): 1, (2, 4): 1}, attach=[(0, 2, 1)], walk=[2],
        out=dict(obs=[[(1, 0), (2, 1)], [(1, 1), (2, 4)]], valid=[1, 1], slots={(1, 0): 0, (1, 1): 1, (2, 1): 0, (2, 4): 1}, result=[2, 4, 2, 0, 1, 0],
                 already=[0], new_pos=[0, 2])),
    "every_skip_reason": dict(  # invalid point; point rows, features, key-frame rows outside the tables; an invalid key-frame; new_kf makes 5 valid
        points=[[(1, 0)], [(1, 1)]], invalid_mp=[1], invalid_kf=[4, 5], new_kf=[5, -1, NKF],
        attach=[(1, 2, 0), (-1, 2, 0), (2, 2, 0), (0, 2, -1), (0, 2, NFK), (0, -1, 0), (0, NKF, 0), (0, 4, 0), (0, 5, 6)], walk=[4],
        out=dict(obs=[[(1, 0), (5, 6)], [(1, 1)]], valid=[1, 0], kf_valid=[1, 1, 1, 1, 0, 1], slots={(1, 0): 0, (1, 1): 1, (5, 6): 0},
                 result=[2, 3, 1, 8, 0, 0], already=[], new_pos=[0, 2])),
}


def hand_scene(table, name):
    sc = table[name]
    m, ba, ref = build(sc["points"], sc.get("invalid_mp", ()), sc.get("invalid_kf", ()), sc.get("mono", ()), sc.get("extra_slots"))
    return dict(sc, m=m, ba=ba, mp_ref_kf=ref)


def new_points(n, seed=5):
    rng = np.random.default_rng(seed)
    return dict(pos=rng.uniform(-5, 5, (n, 3)), assoc=rng.integers(-1, 3000, n).astype(np.int32), ref_kf=rng.integers(0, 4, n).astype(np.int32))


# ---- random scenes: the maps of map_edit_scenes with colliding lists
RANDOM_FUSE = (("tiny", 2), ("small", 1), ("clique", 4))  # (scene, seed): tests/test_map_grow_ref.py asserts each exercises every branch
RANDOM_ADD = (("tiny", 1), ("small", 2), ("clique", 3))
BIG_FUSE, BIG_ADD = ("euroc", 1), ("euroc", 2)  # the rebuild's scan crosses workgroups (180 000 points: 44 tiles)


def _busy_kf(m, but):
    """the valid key-frame that holds the most points among those with four free slots"""
    held = (m["kf_mp"] >= 0).sum(1)
    score = np.where((m["kf_valid"] != 0) & (m["kf_mp"].shape[1] - held >= 4) & (np.arange(len(held)) != but), held, -1)
    assert score.max() > 0
    return int(np.argmax(score))


def fuse_lists(sc, seed, n=None, kf=None):
    """a key-frame and a candidate list for it whose matches collide: most candidates do not observe the key-frame, their best_idx
    falls on a few of its slots - held and empty ones - so that attaches, replaces in both directions and chains follow one another;
    some candidates twice, some invalid / observing / outside the table, some without a match -> (kf, cand_mp, best_idx)"""
    m = sc["m"]
    rng = np.random.default_rng(seed)
    NMP, (NKF_, NFK_) = len(m["mp_valid"]), m["kf_mp"].shape
    if kf is None:
        kf = _busy_kf(m, -1)
    n = min(NMP, 120) if n is None else n
    held = np.nonzero(m["kf_mp"][kf] >= 0)[0]
    free = np.nonzero(m["kf_mp"][kf] < 0)[0]
    pool = np.concatenate([rng.choice(held, min(len(held), 4), replace=False), rng.choice(free, min(len(free), 2), replace=False)])  # ~ n / 6 onto each
    cand = rng.integers(0, NMP, n)
    dup =rng.uniform(size=n) < 0.2
    cand[dup] = rng.choice(cand[~dup], int(dup.sum()))
    best = rng.choice(pool, n)
    best[rng.uniform(size=n) < 0.1] = -1
    cand[:3] = [-1, NMP, 2 ** 31 - 1]
    best[3:5] = [NFK_, -7]
    return kf, cand.astype(np.int32), best.astype(np.int32)


def add_lists(sc, seed, n_new=12, n_extra=40):
    """a key-frame made NEW again - invalid, the CSR forgets it for half of the points it holds - and the additions of one mapping pass:
    new_kf and walk_kf name it (with a duplicate and rows outside the table), n_new new points with two triples each (createMapPoints),
    n_extra colliding triples (duplicates of a pair, several onto one slot, every skip reason) -> (m, ba, mp_ref_kf with the
    key-frame stripped; dict(new_mp, new_kf, attach, walk_kf))"""
    m, ba = {k: np.array(v) for k, v in sc["m"].items()}, {k: (np.array(v) if hasattr(v, "shape") else v) for k, v in sc["ba"].items()}
    rng = np.random.default_rng(seed)
    NMP, (NKF_, NFK_), NOBS = len(m["mp_valid"]), m["kf_mp"].shape, len(m["obs_kf"])
    ok = np.nonzero(m["kf_valid"])[0]
    ok = ok[ok != ba["kf_first"]]
    kf = _busy_kf(m, ba["kf_first"])
    owner = np.repeat(np.arange(NMP), np.diff(m["obs_ptr"]))
    forget = (m["obs_kf"] == kf) & (owner % 2 == 0)
    keep = ~forget
    ptr = np.zeros(NMP + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(owner[keep], minlength=NMP))
    m.update(obs_ptr=ptr.astype(np.int32), obs_kf=m["obs_kf"][keep])
    ba["obs_feat"] = ba["obs_feat"][keep]
    m["kf_valid"][kf] = 0
    ref = ES.first_entry_kf(m)
    free = np.nonzero(m["kf_mp"][kf] < 0)[0]
    others = ok[ok != kf]
    att = []
    for i in range(n_new):  # a new point: the new key-frame and a neighbour, as createMapPoints attaches them
        k2 = int(rng.choice(others))
        f2 = np.nonzero(m["kf_mp"][k2] < 0)[0]
        att += [(NMP + i, kf, int(free[i % len(free)])), (NMP + i, k2, int(f2[i % len(f2)]) if len(f2) else 0)]
    valid = np.nonzero(m["mp_valid"])[0]
    for _ in range(n_extra):
        p, k, f = int(rng.choice(valid)), int(rng.choice(others[:4])), int(rng.integers(0, min(NFK_, 6)))
        att += [(p, k, f)] * int(rng.integers(1, 3))
    bad_mp, bad_kf = np.nonzero(m["mp_valid"] == 0)[0], np.nonzero(m["kf_valid"] == 0)[0]
    att += [(-1, kf, 0), (NMP + n_new, kf, 0), (int(valid[0]), kf, -1), (int(valid[0]), kf, NFK_), (int(valid[0]), -1, 0), (int(valid[0]), NKF_, 0)]
    att += [(int(bad_mp[0]), kf, 0)] if len(bad_mp) else []
    att += [(int(valid[0]), int(k), 1) for k in bad_kf if k != kf][:1]
    order = rng.permutation(len(att))
    att = [att[i] for i in order]
    lists = dict(new_mp=new_points(n_new, seed), new_kf=np.array([kf, -1, NKF_, kf], np.int32), attach=np.array(att, np.int32).reshape(-1, 3),
                 walk_kf=np.array([NKF_, kf, kf, -3], np.int32))
    return m, ba, ref, lists


GROWN = ("small", 2, 1)  # (scene, the seed of its additions, the seed of the fuse list on the grown map): asserted like RANDOM_FUSE


def grown_lists(name=GROWN[0], add_seed=GROWN[1], fuse_seed=GROWN[2]):
    """an add, then a fuse list made ON the map the add leaves (the model's rows) -> dict(m, ba, ref_kf, lists: the add's inputs;
    rows1, res1: the model's add; m1, ba1: the grown map; kf, cand, best: the fuse list)"""
    from tests import map_grow_ref as G
    m, ba, ref_kf, ls = add_lists(ES.scene(name, name in ES.CLAMP), add_seed)
    rows1, res1 = G.map_add(m, ba, ref_kf, ls["new_mp"], ls["new_kf"], ls["attach"], ls["walk_kf"])
    m1, ba1 = G.apply_rows(m, ba, rows1, dict(mp_pos=ls["new_mp"]["pos"]))
    ba1["mp_assoc"] = np.concatenate([ba["mp_assoc"], ls["new_mp"]["assoc"]])
    kf, cand, best = fuse_lists(dict(m=m1, ba=ba1), fuse_seed)
    return dict(m=m, ba=ba, ref_kf=ref_kf, lists=ls, rows1=rows1, res1=res1, m1=m1, ba1=ba1, kf=kf, cand=cand, best=best)


# ---- the geometric scene of the composed pass: real projections, descriptors, twins to merge and observations to find again
GEO_TARGETS = (3, 5, 2)  # the key-frames the new one's points are fused into


def geo_scene(mean, cov, gt, n_twins=90, n_forget=90, seed=77):
    """tests/ba_window_scenes.geometric_scene made ready for searchInNeighbors -> dict(m, ba, kf_row, kf_desc (NKF,NFK,32) u8, mp_ref_kf):
    n_twins points are SPLIT - a twin row at (nearly) the same position takes every second observation, so a search from one finds the
    slot of the other; n_forget points FORGET one observation - the slot is empty, the feature still looks like the point; every
    feature that observes a point carries the point's descriptor with six bits flipped, the others are random."""
    from tests import ba_window_scenes as S
    m, ba, kf_row = S.geometric_scene(mean, cov, gt)
    rng = np.random.default_rng(seed)
    NMP, (NKF_, NFK_) = len(m["mp_valid"]), m["kf_mp"].shape
    ptr = m["obs_ptr"]
    obs = [list(zip(m["obs_kf"][ptr[p]:ptr[p + 1]].tolist(), ba["obs_feat"][ptr[p]:ptr[p + 1]].tolist())) for p in range(NMP)]
    base = rng.integers(0, 256, (NMP, 32)).astype(np.uint8)
    kf_desc = rng.integers(0, 256, (NKF_, NFK_, 32)).astype(np.uint8)
    for p, o in enumerate(obs):
        for k, f in o:
            d = base[p].copy()
            bits = rng.choice(256, 6, replace=False)
            d[bits >> 3] ^= (1 << (bits & 7)).astype(np.uint8)
            kf_desc[k, f] = d
    # the features as the points and poses of the scene project them (the scene's own start a little off, further than the matcher's
    # gates), a fraction of a pixel of noise; the octaves follow the distance as MapPoint::predictScale does (mappoint.cpp:289-293) from
    # the point's first observer, so that the predicted level meets them
    cam = api.Camera()
    kf_uvr, kf_oct = ba["kf_uvr"].copy(), ba["kf_oct"].copy()
    for p, o in enumerate(obs):
        X = m["mp_pos"][p]
        oct_p = int(rng.integers(0, 4))
        for k, f in o:
            T = ba["kf_pose"][k]
            pc = synth.quat_to_R(T[:4]) @ X + T[4:]
            if pc[2] < 0.1:
                continue
            ratio = np.linalg.norm(X - ba["kf_twc"][o[0][0]]) / np.linalg.norm(X - ba["kf_twc"][k])
            oc = int(np.clip(np.round(oct_p + np.log(ratio) / np.log(1.2)), 0, 7))
            sig = 0.3 * 1.2 ** oc
            u, v = cam.fx * pc[0] / pc[2] + cam.cx + rng.standard_normal() * sig, cam.fy * pc[1] / pc[2] + cam.cy + rng.standard_normal() * sig
            ur = u - cam.bf / pc[2] + rng.standard_normal() * sig * 0.5 if kf_uvr[k, f, 2] >= 0 else -1.0
            kf_uvr[k, f] = (u, v, float(np.float32(ur)))
            kf_oct[k, f] = oc
    ba = dict(ba, kf_uvr=kf_uvr, kf_oct=kf_oct)
    many = np.array([p for p in range(NMP) if m["mp_valid"][p] and len(obs[p]) >= 4])
    pick = rng.permutation(many)
    twins, forget = pick[:min(n_twins, len(pick) // 2)], pick[len(pick) // 2:][:n_forget]
    pos, valid, assoc = [m["mp_pos"]], [m["mp_valid"]], [ba["mp_assoc"]]
    kf_mp = m["kf_mp"].copy()
    for p in twins:
        obs.append(obs[p][1::2])
        obs[p] = obs[p][0::2]
        for k, f in obs[-1]:
            kf_mp[k, f] = len(obs) - 1
    pos.append(m["mp_pos"][twins] + rng.standard_normal((len(twins), 3)) * 1e-3)
    valid.append(np.ones(len(twins), np.uint8))
    assoc.append(ba["mp_assoc"][twins])
    for p in forget:
        k, f = obs[p].pop(int(rng.integers(len(obs[p]))))
        kf_mp[k, f] = -1
    optr = np.zeros(len(obs) + 1, np.int32)
    optr[1:] = np.cumsum([len(o) for o in obs])
    m = dict(m, mp_valid=np.concatenate(valid), mp_pos=np.concatenate(pos), kf_mp=kf_mp, obs_ptr=optr, obs_kf=np.array([k for o in obs for k, _ in o], np.int32))
    ba = dict(ba, obs_feat=np.array([f for o in obs for _, f in o], np.int32), mp_assoc=np.concatenate(assoc))
    return dict(m=m, ba=ba, kf_row=int(kf_row), kf_desc=kf_desc, mp_ref_kf=ES.first_entry_kf(m))


def strip_key_frame(m, ba, kf):
    """key-frame kf as the tracking thread hands it over: its kf_mp row filled, no point observes it yet, kf_valid 0 -> (m, ba) copies"""
    NMP = len(m["mp_valid"])
    owner = np.repeat(np.arange(NMP), np.diff(m["obs_ptr"]))
    keep = m["obs_kf"] != kf
    ptr = np.zeros(NMP + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(owner[keep], minlength=NMP))
    kfv = m["kf_valid"].copy()
    kfv[kf] = 0
    return dict(m, obs_ptr=ptr.astype(np.int32), obs_kf=m["obs_kf"][keep], kf_valid=kfv, kf_mp=m["kf_mp"].copy(), mp_valid=m["mp_valid"].copy()), dict(ba, obs_feat=ba["obs_feat"][keep])
